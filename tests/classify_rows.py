"""Constructed rows of known class for every net family: the five-class census (divergent /
fix_zero / fix_other / fix_sec / other) on rows whose class follows from exact arithmetic, not
from a random draw.  tests/test_classify_rows.py (host) and tests/test_classify_rows_gpu.py
(device) demand that every classifier agrees with ``oracle.core.classify`` on EVERY one of them.

Path rows (Weightwise and Recurrent, any width and depth): an all-zero row with
kernel[0][input 0][unit j] = first, kernel[l][j][j] = 1 for the hidden layers,
kernel[last][j][0] = last and every recurrent matrix 0 is the net f(x) = first * last * x, exactly
(every other product is an exact zero).  first * last = -1 gives f(w) = -w: not a fixpoint, but
f(f(w)) = w bitwise -- fix_sec (other without the second-order test); first * last = 1 is the
identity fixpoint.  Self-application F(w) = -w negates every kernel on the path: with an odd
number of kernels (depth 2) -w is the identity, with an even number (depth 1, 3) a negated
identity again -- a row of period 2 that run_fixpoint never leaves (nsteps = steps, class fix_sec).

Constant rows (Aggregating(4, W, D), D even): every weight a = -(0.25 / W**D) ** (1 / (D + 1)), so
that 4 * W**D * a**(D + 1) = -1: the net maps the constant row a to -a and back (residual of the
second application <= 2.3e-8), and the +|a| row is a first-order fixpoint.  Not exact in 16-bit
storage: fp32 only.  For D ODD (Aggregating(4, 10, 3), (4, 4, 3)) NO fix_sec row exists: an output
is constant over each chunk, so a row within eps of its second application is within eps of a
chunk-constant row, and on constant rows the net multiplies by 4 * W**D * a**(D + 1) with D + 1
even, which cannot be negative -- a second-order fixpoint is a first-order one there.  Those shapes
reach the fix_sec branch with a NEGATIVE result only (the rows that are other with the
second-order test on); both constant rows, +a and -a, are first-order fixpoints there.

Preimages (the big aggregating nets): a non-constant row u whose first self-application is the
constant a row (tests/golden/classify_preimage_*.npy, found by ``solve_preimage``): the chunk-state
kernels classify the state AFTER the first step, so run_fixpoint(steps=1) of u is fix_sec.

Boundary rows: an all-zero row has a zero last layer, f == 0 under any contraction, so entry 1 = t
decides |0 - t| >= eps alone: t = eps is NOT close (the reference's strict test), nextafter(eps, 0)
is.  Edge rows: a dead weight next to the identity, a finite row whose application overflows
(other, not divergent), +inf / NaN in the row (divergent), a row of -0.0 (fix_zero).

``margins`` evaluates in float64 max|f(w) - w|, max|f(f(w)) - w| and max|w| of every row and
``check_margins`` asserts each is below eps / 4 or above 4 * eps (non-finite counts as above); the
boundary rows are exempt by name and their applications asserted to be exactly 0.  That is what
justifies 0 mismatches: no fma contraction moves a row across eps.

Populations: ``population(rows, n, rot)`` tiles the rows so that row i has class (i + rot) % 5 --
every class at row 0 and at row n - 1 over the rotations -- and, from 128 rows on, rows 64..127 are
one class (a full 64-row ballot block).  n = 257 leaves one wave in k_wide's last 4-wave block and
a partial ballot block.  A population of one row has one class; every other one shows all five
(four for the odd-depth aggregating shapes, see above)."""
import functools
import os

import numpy as np
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.oracle import core as O
from self_replicating_neural_networks_amd.soup_engine import SoupEngine

EPS = np.float32(1e-4)
SIZES = (1, 63, 64, 65, 257)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

WW, RNN, AGG = ArchSpec.weightwise, ArchSpec.recurrent, ArchSpec.aggregating
LANE = [WW(2, 2), WW(4, 3), AGG(4, 2, 2), AGG(4, 2, 2, shuffler="random"), RNN(2, 2)]
FIX_GROUP = [WW(2, 2), WW(2, 1), WW(1, 1)]
GENERIC = [WW(3, 3), WW(10, 3), RNN(3, 2), AGG(4, 4, 3)]
RNN_WAVE = [RNN(8, 2), RNN(16, 2), RNN(8, 3)]
WIDE = [WW(16, 2), WW(16, 3), WW(32, 2)]
BIG = [AGG(4, 8, 2), AGG(4, 8, 2, aggregator="max"), AGG(4, 16, 2), AGG(4, 10, 3)]
PREIMAGE = BIG[:3]


def sid(s):
    tag = {"weightwise": "ww", "recurrent": "rnn", "aggregating": "agg"}[s.kind]
    return f"{tag}-{s.width}-{s.depth}" + ("-max" if s.aggregator == "max" else "") + \
        ("-shuf" if s.shuffler == "random" else "")


def has_fix_sec(spec):
    """False for the odd-depth aggregating shapes (module docstring): four classes only"""
    return not (spec.kind == "aggregating" and spec.depth % 2 == 1)


# ------------------------------------------------------------------------------ the rows
def _kernels(spec):
    """(offset, rows, cols) of the feed-forward kernels (the recurrent matrices left out)"""
    ks = list(zip(spec.offsets, spec.layer_shapes))
    if spec.kind == "recurrent":
        ks = ks[0::2]
    return [(o, r, c) for o, (r, c) in ks]


def path_row(spec, first, last, j):
    w = np.zeros(spec.P, dtype=np.float32)
    ks = _kernels(spec)
    o, _, c = ks[0]
    w[o + 0 * c + j] = first
    for o, _, c in ks[1:-1]:
        w[o + j * c + j] = 1.0
    o, _, c = ks[-1]
    w[o + j * c + 0] = last
    return w


def agg_a(spec):
    return np.float32((0.25 / spec.width ** spec.depth) ** (1.0 / (spec.depth + 1)))


@functools.lru_cache(maxsize=None)
def preimage(spec):
    """The stored non-constant row whose first self-application is the constant -|a| row"""
    return np.load(os.path.join(GOLDEN, f"classify_preimage_{sid(spec).replace('-', '_')}.npy"))


def solve_preimage(spec, seed=0, iters=40):
    """Gauss-Newton in float64 from 0.3 * randn on the ``aggregates`` equations
    apply(u, u)[chunk starts] = -|a| (minimum-norm steps, numerical Jacobian): a fixed seed and a
    fixed iteration count; the float32 rounding of the result"""
    rng = np.random.default_rng(seed)
    u = 0.3 * rng.standard_normal(spec.P)
    starts = [s for s, _ in spec.chunks]
    target = -float(agg_a(spec))
    res = lambda v: apply64(spec, v, v)[starts] - target
    for _ in range(iters):
        r = res(u)
        J = np.empty((len(starts), spec.P))
        for k in range(spec.P):
            d = np.zeros(spec.P)
            d[k] = 1e-6
            J[:, k] = (res(u + d) - res(u - d)) / 2e-6
        u = u - np.linalg.lstsq(J, r, rcond=None)[0]
    return u.astype(np.float32)


BOUNDARY = ("zero+eps", "zero+below_eps", "zero+above_eps", "zero-eps")


@functools.lru_cache(maxsize=None)
def rows_of(spec):
    """[(name, row float32[P])] for ``spec``; the names of BOUNDARY are the exact-arithmetic
    boundary rows"""
    P = spec.P
    out = []
    z = np.zeros(P, dtype=np.float32)

    def at(base, k, v):
        w = base.copy()
        w[k] = v
        return w

    ident = None
    if spec.kind in ("weightwise", "recurrent"):
        for j in sorted({0, spec.width - 1}):
            out += [(f"negid{j}", path_row(spec, -1.0, 1.0, j)), (f"ident{j}", path_row(spec, 1.0, 1.0, j)),
                    (f"pow2_{j}", path_row(spec, -4.0, 0.25, j)), (f"overflow{j}", path_row(spec, 1e20, 1e20, j))]
        ident = path_row(spec, 1.0, 1.0, 0)
        if spec.kind == "weightwise" and spec.width >= 2:
            dead = 3 * spec.width + spec.width - 1  # A0[3][W-1]: a unit nothing reads
            out += [("ident+dead_eps", at(ident, dead, EPS)), ("ident+dead_half", at(ident, dead, 0.5))]
            neg = path_row(spec, -1.0, 1.0, 0)
            rng = np.random.default_rng(4321)
            for sc, tag in ((1e-6, "negid~1e-6"), (1e-2, "negid~1e-2")):
                # the first 64 draws that pass the margin guard: about 1 in 50 of the 1e-2 draws has a
                # path gain k with |k * k - 1| between eps / 4 and 4 * eps and is left out
                noise = rng.standard_normal((256, P)).astype(np.float32)
                keep = []
                for q in range(256):
                    if len(keep) < 64 and _decided(spec, neg + np.float32(sc) * noise[q]):
                        keep.append(q)
                assert len(keep) == 64
                out += [(f"{tag}#{i}", neg + np.float32(sc) * noise[q]) for i, q in enumerate(keep)]
    else:
        a = agg_a(spec)
        ident = np.full(P, a, dtype=np.float32)
        out += [("const-a", np.full(P, -a, dtype=np.float32)), ("const+a", ident)]
        if spec.P > 64 and spec.depth % 2 == 0 and spec.shuffler == "none":
            out.append(("preimage", preimage(spec)))
    out += [("zero+eps", at(z, 1, EPS)), ("zero+below_eps", at(z, 1, np.nextafter(EPS, np.float32(0)))),
            ("zero+above_eps", at(z, 1, np.nextafter(EPS, np.float32(1)))), ("zero-eps", at(z, 1, -EPS)),
            ("zero+5", at(z, 1, 5.0)), ("zero", z), ("negzero", np.full(P, -0.0, dtype=np.float32)),
            ("fix+inf", at(ident, min(5, P - 2), np.inf)), ("fix+nan", at(ident, P - 1, np.nan))]
    return out


# classes the issue's tables give, (with_sec, without): every other row is checked against the oracle only
TABLE = {"negid": (3, 4), "ident": (2, 2), "pow2_": (3, 4), "overflow": (4, 4), "negid~1e-6": (3, 4),
         "negid~1e-2": (4, 4), "const-a": (3, 4), "const+a": (2, 2), "preimage": (4, 4), "zero+eps": (4, 4),
         "zero+below_eps": (1, 1), "zero+above_eps": (4, 4), "zero-eps": (4, 4), "zero+5": (4, 4), "zero": (1, 1),
         "negzero": (1, 1), "fix+inf": (0, 0), "fix+nan": (0, 0)}


def table_class(spec, name, with_sec=True):
    key = max((k for k in TABLE if name.startswith(k)), key=len)
    if key == "const-a" and not has_fix_sec(spec):
        return 2  # (D + 1 even: the gain of the -a row is +1 as well)
    return TABLE[key][0 if with_sec else 1]


@functools.lru_cache(maxsize=None)
def base(spec):
    """(names, rows [m, P], oracle classes with the second-order test, without)"""
    names, rows = zip(*rows_of(spec))
    rows = np.stack(rows)
    return list(names), rows, O.classify(spec, rows, EPS, True), O.classify(spec, rows, EPS, False)


@functools.lru_cache(maxsize=None)
def base_run(spec, steps, early_exit, with_sec=True):
    """oracle run_fixpoint of the run rows of ``spec``: (final rows, nsteps, classes)"""
    return O.run_fixpoint(spec, base(spec)[1][run_rows(spec, early_exit)], steps, EPS, early_exit, with_sec)


def run_rows(spec, early_exit=True):
    """indices of the rows a run_fixpoint comparison uses: every row but the randomly perturbed
    ones, whose later steps no margin guard covers.  Without the early exit the rows of the
    aggregating nets that are not exact in float32 are left out as well: the constant fixpoint
    repels (the self-application map s -> c * s**(D + 1) has slope D + 1 there), so seven steps
    carry a rounding error of 1e-8 to the size of eps, differently in every summation order; with
    the early exit those rows stop after at most two steps."""
    skip = ("~",) if early_exit or spec.kind != "aggregating" else ("~", "const", "preimage")
    return np.array([i for i, nm in enumerate(base(spec)[0]) if not any(s in nm for s in skip)])


def lowp_rows(spec, dtype):
    """indices of the rows a 16-bit table stores exactly (the path rows, zeros, inf, NaN)"""
    rows = torch.from_numpy(base(spec)[1])
    back = rows.to(dtype).float()
    same = ((back == rows) | (back.isnan() & rows.isnan())).all(dim=1)
    return np.nonzero(same.numpy())[0]


# ------------------------------------------------------------------------------ float64 margins
def apply64(spec, a, t):
    """f_a(t) of one particle in float64 (unshuffled: callers pass rows whose output is constant
    where the net shuffles)"""
    a, t = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)
    mats = [a[o:o + r * c].reshape(r, c) for (r, c), o in zip(spec.layer_shapes, spec.offsets)]
    with np.errstate(all="ignore"):
        if spec.kind == "weightwise":
            h = np.concatenate([t[:, None], spec.coords().astype(np.float64)], axis=1)
            for m in mats:
                h = h @ m
            return h[:, 0]
        if spec.kind == "aggregating":
            g = np.array([t[s:s + L].mean() if spec.aggregator == "mean" else t[s:s + L].max() for s, L in spec.chunks])
            for m in mats:
                g = g @ m
            out = np.empty(spec.P)
            for k, (s, L) in enumerate(spec.chunks):
                out[s:s + L] = g[k]
            return out
        hs = [np.zeros(m.shape[1]) for m in mats[0::2]]
        out = np.empty(spec.P)
        for i in range(spec.P):
            x = t[i:i + 1]
            for l in range(len(hs)):
                hs[l] = x @ mats[2 * l] + hs[l] @ mats[2 * l + 1]
                x = hs[l]
            out[i] = x[0]
        return out


def margins(spec, w):
    """(max|f(w) - w|, max|f(f(w)) - w|, max|w|) in float64; inf where not finite"""
    with np.errstate(all="ignore"):
        f1 = apply64(spec, w, w)
        f2 = apply64(spec, w, f1)
        q = [np.max(np.abs(f1 - w)), np.max(np.abs(f2 - w)), np.max(np.abs(w.astype(np.float64)))]
    return [float(v) if np.isfinite(v) else float("inf") for v in q]


def _decided(spec, w):
    return all(v < float(EPS) / 4 or v > 4 * float(EPS) for v in margins(spec, w))


def check_margins(spec):
    """the guard of the module docstring on every row of ``spec``"""
    eps = float(EPS)
    for name, w in rows_of(spec):
        if name in BOUNDARY:
            f1 = O.apply(spec, w[None], w[None])
            f2 = O.apply(spec, w[None], f1)
            assert not f1.any() and not f2.any(), name
            continue
        if spec.shuffler == "random":  # (the shuffle moves nothing that differs)
            f1 = apply64(spec, w, w)
            assert np.all(f1 == f1[0]) or not np.all(np.isfinite(f1)), name
        for v in margins(spec, w):
            assert v < eps / 4 or v > 4 * eps, (sid(spec), name, v)


# ------------------------------------------------------------------------------ populations
def population(spec, n, rot, rows=None, with_sec=True):
    """indices [n] into the rows of ``spec`` (module docstring); ``rows``: restrict to these row
    indices (default: all).  Classes by the oracle with the second-order test."""
    cls = base(spec)[2]
    pool = np.arange(len(cls)) if rows is None else np.asarray(rows)
    by = {c: [i for i in pool if cls[i] == c] for c in range(5)}
    live = [c for c in range(5) if by[c]]
    used = {c: 0 for c in live}
    idx = np.empty(n, dtype=np.int64)

    def take(c):
        used[c] += 1
        return by[c][(used[c] - 1) % len(by[c])]

    for i in range(n):
        idx[i] = take(live[(i + rot) % len(live)])
    if n >= 128:
        for i in range(64, 128):
            idx[i] = take(live[rot % len(live)])
    return idx


def populations(spec, sizes=SIZES, rows=None):
    """[(n, rot, idx)] over the sizes and the five rotations"""
    return [(n, rot, population(spec, n, rot, rows)) for n in sizes for rot in range(5)]


def table(spec, idx, device="cpu", dtype=torch.float32):
    """the weight table [n, PP] of a population"""
    W = torch.zeros((len(idx), spec.PP), dtype=torch.float32)
    W[:, :spec.P] = torch.from_numpy(base(spec)[1][idx])
    return W.to(dtype).to(device)


def n_classes(spec):
    return 5 if has_fix_sec(spec) else 4


def histogram(cls):
    return np.bincount(np.asarray(cls, dtype=np.int64), minlength=5)


# ------------------------------------------------------------------------------ static soups
STATIC = dict(attacking_rate=0.0, learn_from_rate=0.0, train=0, remove_divergent=False, remove_zero=False,
              epsilon=float(EPS))


def check_static_soup(spec, dev, order="synchronous", fused=None, graph=False, route=None):
    """nobody attacks, learns, trains or is removed: after evolve(1) and evolve(3) the rows are
    bitwise the constructed ones and last_census() == count() == the oracle's histogram, with the
    second-order test and without"""
    _, _, c1, c0 = base(spec)
    for n, rot in ((65, 1), (257, 3)):
        idx = population(spec, n, rot)
        rows = table(spec, idx)
        for with_sec, want in ((True, c1[idx]), (False, c0[idx])):
            e = SoupEngine(spec, n, STATIC, device=dev, seed=5, order=order, weights=rows[:, :spec.P])
            e.stats = True
            e.stats_with_sec = with_sec
            if fused is not None:
                e.fused = fused
            if route is not None:
                route(e)
            if graph:
                assert e.capture(warmup=1)
            hist = O.counts_of(want)
            assert sum(v > 0 for v in hist.values()) == n_classes(spec) - (has_fix_sec(spec) and not with_sec)
            for k in (1, 3):
                e.evolve(k)
                assert e.last_census() == hist, (n, with_sec, k, e.last_census(), hist)
                assert e.count(with_sec=with_sec) == hist
                got = e.local_rows().cpu().contiguous()
                assert torch.equal(got.view(torch.int32), rows.view(torch.int32)), (n, k)
            if order == "sequential":
                assert e.ordered_levels()["error"] == 0
            e.release_graphs()
