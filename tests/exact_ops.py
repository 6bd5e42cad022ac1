"""The four ops of a particle table against the exact float32 oracle (oracle/exact.py) at zero
tolerance, on the host path (tests/test_exact_oracle.py) and on every device kernel route
(tests/test_exact_families_gpu.py): an attack through the three gathers, run_fixpoint without
early exit, self-train epochs with their loss, and learn_from through a teacher gather.

Every comparison is on bit patterns: infinities and signed zeros must match, NaNs only as NaNs
(payloads are not a contract).  Aggregating rows come from the engine's init on the table's
device, which must itself equal the oracle's; Recurrent rows are the host init scaled by 0.5
(no exact init: the orthogonal kernels go through libm), at which every row stays finite
through these ops -- ``check_ops`` asserts that share, so a comparison never runs on inf / NaN
patterns alone."""
import numpy as np
import torch

from self_replicating_neural_networks_amd.oracle import exact as X
from self_replicating_neural_networks_amd.ops import kernels as K

SEED, UID0, LR = 7, 5, 0.01


def bits(a):
    """int32 bit patterns with every NaN mapped to one pattern."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return np.where(np.isnan(a), np.int32(0x7FC00000), a.view(np.int32))


def assert_bits(got, exp, what):
    g, e = bits(got), bits(exp)
    bad = g != e
    if bad.any():
        rows = np.unique(np.nonzero(bad.reshape(bad.shape[0], -1))[0])
        r = int(rows[0])
        raise AssertionError(f"{what}: {rows.size} of {bad.shape[0]} rows differ from the exact oracle, first row {r}: "
                             f"got {np.asarray(got, dtype=np.float32)[r].ravel()[:6]} "
                             f"want {np.asarray(exp, dtype=np.float32)[r].ravel()[:6]}")


def finite_share(a) -> float:
    a = np.asarray(a, dtype=np.float32)
    return float(np.mean(np.all(np.isfinite(a.reshape(a.shape[0], -1)), axis=1)))


def gathers(n):
    """idx_f / idx_t / idx_o of an attack: entry 0 is an identity entry (f = t = o = 0), entries 1
    and 2 share one attacker; idx_o is a permutation (every output row written once)."""
    if n < 3:
        z = np.zeros(n, dtype=np.int64)
        return z, z.copy(), np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(n)
    idx_f = rng.permutation(n)
    idx_t = rng.permutation(n)
    idx_o = np.roll(np.arange(n), -1)
    idx_o[[0, n - 1]] = 0, 1  # still a permutation: 0 -> 0, n-1 -> 1 (the roll sent 0 -> 1, n-1 -> 0)
    idx_f[0] = idx_t[0] = 0
    idx_f[2] = idx_f[1]
    return idx_f.astype(np.int64), idx_t.astype(np.int64), idx_o.astype(np.int64)


def teachers(n):
    """idx_t of a learn_from: entry 0 learns from itself, entries 1 and 2 from the same teacher."""
    idx = np.roll(np.arange(n), 3)
    idx[0] = 0
    if n > 2:
        idx[2] = idx[1]
    return idx.astype(np.int64)


def start_rows(spec, n, dev):
    """(table [n, PP] on ``dev``, its rows as numpy, uid tensor, uid numpy)."""
    uid = torch.arange(n, dtype=torch.int64) + UID0
    if spec.kind == "recurrent":
        W = torch.zeros(n, spec.PP)
        K.init_rows(spec, W, uid, SEED)
        W = (W * 0.5).to(dev)
    else:
        W = torch.zeros(n, spec.PP, device=dev)
        K.init_rows(spec, W, uid.to(dev), SEED)
        assert_bits(W[:, :spec.P], X.init(spec, uid.numpy(), SEED), f"{spec} init")
    return W, W[:, :spec.P].cpu().numpy().copy(), uid.to(dev), uid.numpy().astype(np.uint64)


def check_attack(spec, W, w0, uid, uids):
    n, dev = W.shape[0], W.device
    out = torch.zeros_like(W)
    K.apply(spec, W, out, uid=uid, seed=SEED, ctr=2)  # one self-application, no gather
    assert_bits(out[:, :spec.P], X.apply(spec, w0, w0, SEED, uids, 2), f"{spec} self-application")
    f, t, o = gathers(n)
    out = torch.zeros_like(W)
    K.apply(spec, W, out, idx_f=torch.from_numpy(f).to(dev), idx_t=torch.from_numpy(t).to(dev),
            idx_o=torch.from_numpy(o).to(dev), uid=uid, seed=SEED, ctr=3)
    exp = np.empty_like(w0)
    exp[o] = X.apply(spec, w0[f], w0[t], SEED, uids[t], 3)  # shuffle_random is keyed by the target's uid
    assert finite_share(exp) >= 0.9
    assert_bits(out[:, :spec.P], exp, f"{spec} attack")


def check_fixpoint(spec, W, w0, uid, uids, steps=3):
    T = W.clone()
    _, nsteps, _ = K.run_fixpoint(spec, T, steps, 1e-4, early_exit=False, uid=uid, seed=SEED, ctr=20)
    exp = w0
    for s in range(steps):
        exp = X.apply(spec, exp, exp, SEED, uids, 20 + s)
    assert finite_share(exp) >= 0.9
    assert np.array_equal(nsteps.cpu().numpy(), np.full(W.shape[0], steps))
    assert_bits(T[:, :spec.P], exp, f"{spec} run_fixpoint({steps})")


def check_train(spec, W, w0, uid, uids, epochs=3):
    T = W.clone()
    loss = K.train(spec, T, epochs=epochs, lr=LR, uid=uid, seed=SEED, ctr=11)
    exp, el = X.train_epochs(spec, w0, None, epochs, True, lr=LR, seed=SEED, uids=uids, ctr=11)
    assert finite_share(exp) >= 0.9
    assert_bits(T[:, :spec.P], exp, f"{spec} train({epochs})")
    assert_bits(loss, el, f"{spec} train({epochs}) loss")


def check_learn(spec, W, w0, uid, uids, epochs=2):
    n, dev = W.shape[0], W.device
    idx = teachers(n)
    L = W.clone()
    loss = K.learn_from(spec, L, W, idx_t=torch.from_numpy(idx).to(dev), epochs=epochs, lr=LR, uid=uid, seed=SEED,
                        ctr=5)
    exp, el = X.train_epochs(spec, w0, w0[idx], epochs, False, lr=LR, seed=SEED, uids=uids, ctr=5)
    assert finite_share(exp) >= 0.9
    assert_bits(L[:, :spec.P], exp, f"{spec} learn_from({epochs})")
    assert_bits(loss, el, f"{spec} learn_from({epochs}) loss")


CHECKS = {"attack": check_attack, "fixpoint": check_fixpoint, "train": check_train, "learn": check_learn}


def check_ops(spec, n, dev, ops=tuple(CHECKS)):
    W, w0, uid, uids = start_rows(spec, n, dev)
    for op in ops:
        CHECKS[op](spec, W, w0, uid, uids)
        assert_bits(W[:, :spec.P], w0, f"{spec} input table after {op}")
