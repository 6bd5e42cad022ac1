"""Trajectory recording of run_fixpoint on host tables: the dense form for the big aggregating
nets (runtime-shape engine), the compact chunk-state form, and run_population on top of it.

The input recipe (``make_rows``) and the comparison helpers are shared with
tests/test_trajectory_record_gpu.py."""
import numpy as np
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.experiment import FixpointExperiment
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.population import Population

N, STEPS, EPS = 333, 6, 1e-4  # 333 rows: more than one 256-row block, a full wave and a 13-lane wave in the last
AGG = ArchSpec.aggregating(4, 10, 3)


def make_rows(spec, n=N, device="cpu", dtype=torch.float32):
    """Rows that stop at different steps: zero, NaN and inf rows (step 0), shrunk rows that converge
    to zero at different speeds, blown-up rows, the rest fresh."""
    W = torch.zeros(n, spec.PP, device=device)
    K.init_rows(spec, W, torch.arange(n, dtype=torch.int64, device=device) + 3, 5)
    W[0:8] = 0
    W[8:12, :spec.P] = float("nan")
    W[12:16, 0] = float("inf")
    W[16:80] *= 0.05
    W[80:140] *= 0.3
    W[140:200] *= 3.0
    return W.to(dtype).contiguous()


def canon(t):
    """Bit pattern of a tensor with every NaN mapped to one value (NaN payloads are not a contract)."""
    t = torch.nan_to_num(t.float(), 7.0, 9.0, -9.0).contiguous()
    return t.view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(canon(a), canon(b))


def exercises_early_exit(nsteps):
    """the returned step counts take at least three distinct values including 0"""
    v = set(nsteps.cpu().tolist())
    return 0 in v and len(v) >= 3


def stepwise_chain(spec, W, steps, eps, early_exit, uid=None, seed=0, ctr=0, via_float=False):
    """The dense trajectory from one-step launches: run_fixpoint(steps=1, early_exit=False) on the
    rows that had not stopped; a row stops where run_net's tests say so (one more one-step launch
    WITH early exit takes no step exactly then).  A row's k-th step runs with op counter ctr + k - 1,
    as inside one launch.  ``via_float``: the step of a 16-bit table is a float32 step rounded to
    the storage format."""
    n = W.shape[0]
    traj = torch.zeros((steps + 1, n, spec.PP), dtype=W.dtype, device=W.device)
    traj[0] = W
    cur = W.clone()
    alive = torch.ones(n, dtype=torch.bool, device=W.device)
    nsteps = torch.zeros(n, dtype=torch.int32, device=W.device)
    for s in range(1, steps + 1):
        kw = dict(uid=uid, seed=seed, ctr=ctr + s - 1)
        if early_exit:
            probe = cur.clone()
            _, took, _ = K.run_fixpoint(spec, probe, 1, eps, early_exit=True, **kw)
            alive &= took == 1
        nxt = cur.to(torch.float32, copy=True) if via_float else cur.clone()
        K.run_fixpoint(spec, nxt, 1, eps, early_exit=False, **kw)
        nxt = nxt.to(W.dtype)
        cur = torch.where(alive[:, None], nxt, cur)
        traj[s] = torch.where(alive[:, None], nxt, torch.zeros_like(nxt))
        nsteps += alive.to(torch.int32)
    return traj, cur, nsteps


def check_history(exp, pop, dense, nsteps):
    """historical_particles[uid]: nsteps + 1 states minus the non-finite ones, weights of the dense
    recording, time = step"""
    dense, nsteps = dense.float().cpu().numpy(), nsteps.cpu().numpy()
    P = pop.spec.P
    for r, uid in enumerate(pop.uid.cpu().tolist()):
        states = exp.historical_particles[uid]
        keep = [0] + [s for s in range(1, int(nsteps[r]) + 1) if np.all(np.isfinite(dense[s, r, :P]))]
        assert [st["time"] for st in states] == keep
        for st in states:
            got, want = st["weights"], dense[st["time"], r, :P]
            assert got.dtype == np.float32 and got.shape == (P,)
            assert np.array_equal(np.nan_to_num(got, nan=7.0).view(np.int32), np.nan_to_num(want, nan=7.0).view(np.int32))


@pytest.mark.parametrize("early_exit", [True, False])
def test_big_aggregating_host_table_records_the_stepwise_chain(early_exit):
    W0 = make_rows(AGG)
    W = W0.clone()
    cls, nsteps, traj = K.run_fixpoint(AGG, W, STEPS, EPS, early_exit=early_exit, record=True)
    assert traj.shape == (STEPS + 1, N, AGG.PP)
    if early_exit:
        assert exercises_early_exit(nsteps)
        assert np.bincount(nsteps.numpy(), minlength=STEPS + 1).tolist() == [16, 98, 147, 30, 42, 0, 0]
    ref, last, ref_steps = stepwise_chain(AGG, W0, STEPS, EPS, early_exit)
    assert torch.equal(nsteps, ref_steps)
    assert same(traj, ref) and same(W, last)
    Wn = W0.clone()
    cls_n, nsteps_n, none = K.run_fixpoint(AGG, Wn, STEPS, EPS, early_exit=early_exit)
    assert none is None and same(Wn, W) and torch.equal(cls_n, cls) and torch.equal(nsteps_n, nsteps)


@pytest.mark.parametrize("spec", [ArchSpec.aggregating(4, 2, 2), AGG], ids=["agg4_2_2", "agg4_10_3"])
@pytest.mark.parametrize("early_exit", [True, False])
def test_state_form_on_host_equals_dense(spec, early_exit):
    W0 = make_rows(spec)
    Wd, Ws = W0.clone(), W0.clone()
    cls_d, nsteps_d, dense = K.run_fixpoint(spec, Wd, STEPS, EPS, early_exit=early_exit, record=True)
    cls_s, nsteps_s, st = K.run_fixpoint(spec, Ws, STEPS, EPS, early_exit=early_exit, record="state")
    if early_exit:
        assert exercises_early_exit(nsteps_d)
    assert isinstance(st, K.StateTrajectory)
    assert st.states.shape == (STEPS, N, spec.aggregates) and st.states.dtype == torch.float32
    assert same(st.row0, W0) and torch.equal(st.nsteps, nsteps_d)
    assert same(st.full(), dense)
    assert same(Ws, Wd) and torch.equal(cls_s, cls_d) and torch.equal(nsteps_s, nsteps_d)
    starts = [c[0] for c in spec.chunks]
    assert same(st.states, dense[1:, :, starts])
    for s in (0, 1, STEPS):
        assert same(st.rows(s), dense[s])
    for r in (0, 9, 100, N - 1):
        k = int(nsteps_d[r])
        got = st.particle(r)
        assert got.shape == (k + 1, spec.P)
        assert same(torch.from_numpy(got), dense[:k + 1, r, :spec.P])


def test_state_form_single_row():
    W0 = make_rows(AGG)[100:101].contiguous()
    Wd, Ws = W0.clone(), W0.clone()
    _, nsteps, dense = K.run_fixpoint(AGG, Wd, STEPS, EPS, record=True)
    _, _, st = K.run_fixpoint(AGG, Ws, STEPS, EPS, record="state")
    assert int(nsteps[0]) > 0 and same(st.full(), dense) and same(Ws, Wd)


def test_state_form_needs_an_unshuffled_aggregating_net():
    for spec in (ArchSpec.weightwise(2, 2), ArchSpec.aggregating(4, 2, 2, shuffler="random")):
        with pytest.raises(ValueError, match="state"):
            K.run_fixpoint(spec, torch.zeros(4, spec.PP), 2, EPS, record="state")
    with pytest.raises(ValueError, match="record"):
        K.run_fixpoint(AGG, torch.zeros(4, AGG.PP), 2, EPS, record="dense")


def test_run_population_records_the_big_aggregating_net_on_host():
    W0 = torch.cat([make_rows(AGG)[[0, 8, 12]], make_rows(AGG)[[20, 100, 150, 250, 300]]])
    pop = Population(AGG, 8, weights=W0, uid_start=40)
    ref = W0.clone()
    _, nsteps, dense = K.run_fixpoint(AGG, ref, STEPS, EPS, record=True)
    exp = FixpointExperiment()
    counts = exp.run_population(pop, STEPS, record=True)
    assert sum(counts.values()) == 8 and same(pop.W, ref)
    assert sorted(exp.historical_particles) == list(range(40, 48))
    check_history(exp, pop, dense, nsteps)
