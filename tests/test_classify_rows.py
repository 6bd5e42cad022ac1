"""Every host classifier on the constructed rows of tests/classify_rows.py: 0 mismatches with
``oracle.core.classify`` / ``run_fixpoint``, not 99 % agreement on random rows.

The host path runs the same C++ as the device for the lane templates and the runtime-shape engine;
the fix_sec branch of each implementation is reached with a POSITIVE result by

  classify_w (csrc/srnn_kernels.h)   test_host_classify[ww-2-2 .. rnn-2-2] (Item::classify) and
                                     test_host_run_fixpoint (Item::run_fixpoint): the negated
                                     identities, the (-4, 0.25) rows, the constant -a rows
  g_classify_w (csrc/srnn_generic.hip)  test_host_classify / test_host_run_fixpoint of the runtime
                                     shapes, the wide and the big nets (the host serves every one of them
                                     on the runtime-shape engine)

k_fix_group, pair::classify, rw_classify, wide_classify and the classifiers of csrc/srnn_bignet.h
have no host form: tests/test_classify_rows_gpu.py.  (The packed class counts of the reference
order's close have a host form of their own: test_host_static_soup_census[*-sequential] and
tests/test_ordered_census.py.)  The odd-depth aggregating shapes
(Aggregating(4, 4, 3), (4, 10, 3)) reach the branch with a negative result only: no fix_sec row
exists for them (tests/classify_rows.py)."""
import numpy as np
import pytest
import torch

import classify_rows as R
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.oracle import core as O

EPS = float(R.EPS)
SPECS = []
for _group in (R.LANE, R.FIX_GROUP, R.GENERIC, R.RNN_WAVE, R.WIDE, R.BIG):
    SPECS += [s for s in _group if s not in SPECS]


@pytest.mark.parametrize("spec", SPECS, ids=R.sid)
def test_rows_have_the_tabled_classes_and_margins(spec):
    """the oracle gives every named row the class the construction predicts, with and without the
    second-order test, and no decision of a non-boundary row lies within a factor 4 of eps"""
    names, rows, c1, c0 = R.base(spec)
    for k, name in enumerate(names):
        assert (c1[k], c0[k]) == (R.table_class(spec, name, True), R.table_class(spec, name, False)), name
    R.check_margins(spec)
    assert sum(R.histogram(c1) > 0) == R.n_classes(spec)
    if R.has_fix_sec(spec):  # without the second-order test every fix_sec row is counted as other
        assert R.histogram(c0)[3] == 0 and R.histogram(c0)[4] == R.histogram(c1)[3] + R.histogram(c1)[4]


@pytest.mark.parametrize("spec", [s for s in SPECS if s.kind != "aggregating"], ids=R.sid)
def test_self_application_negates_a_path_row(spec):
    """F(w) = -w bitwise: the identity after one step with three kernels on the path, period 2 with
    two or four (run_fixpoint never exits early: nsteps = steps, the final row -w, class fix_sec)"""
    for j in sorted({0, spec.width - 1}):
        w = R.path_row(spec, -1.0, 1.0, j)[None]
        assert np.array_equal(O.apply(spec, w, w), -w)
        end, ns, cls = O.run_fixpoint(spec, w, 7, R.EPS, early_exit=True)
        assert np.array_equal(end, -w)
        if spec.depth % 2 == 0:  # (-1)**3 = -1: -w computes f(x) = x
            assert (int(ns[0]), int(cls[0])) == (1, O.C_FIX_OTHER) and np.array_equal(O.apply(spec, end, end), end)
        else:
            assert (int(ns[0]), int(cls[0])) == (7, O.C_FIX_SEC)


def _supported(spec, op):
    assert _lib.supports(spec, op, device=False), f"no host path for {R.sid(spec)}"


@pytest.mark.parametrize("spec", SPECS, ids=R.sid)
def test_host_classify(spec):
    _supported(spec, _lib.OP_CLASSIFY)
    _, _, c1, c0 = R.base(spec)
    for n, rot, idx in R.populations(spec):
        W = R.table(spec, idx)
        before = W.clone()
        for with_sec, want in ((True, c1[idx]), (False, c0[idx])):
            cls, counts = K.classify(spec, W, EPS, with_sec=with_sec)
            bad = np.nonzero(cls.numpy() != want)[0]
            assert bad.size == 0, [(R.base(spec)[0][idx[i]], int(cls[i]), int(want[i])) for i in bad[:8]]
            assert np.array_equal(counts.numpy(), R.histogram(want))
        if n > 1:
            assert sum(R.histogram(c1[idx]) > 0) == R.n_classes(spec)
        assert torch.equal(W.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("spec", SPECS, ids=R.sid)
def test_host_run_fixpoint(spec):
    """7 steps with and without the early exit, and 0 steps (the classifier of the run alone, on
    every row)"""
    _supported(spec, _lib.OP_RUN_FIXPOINT)
    for early in (True, False):
        rr = R.run_rows(spec, early)
        where = {int(r): k for k, r in enumerate(rr)}
        end, ns, cls = R.base_run(spec, 7, early)
        for n, rot, idx in R.populations(spec, sizes=(65,), rows=rr):
            sel = np.array([where[int(i)] for i in idx])
            W = R.table(spec, idx)
            gc, gn, _ = K.run_fixpoint(spec, W, 7, EPS, early_exit=early)
            assert np.array_equal(gc.numpy(), cls[sel]) and np.array_equal(gn.numpy(), ns[sel])
            if R.has_fix_sec(spec) and spec.depth % 2 == 1:
                assert (cls[sel] == O.C_FIX_SEC).any()  # the period-2 rows end as fix_sec
    _, _, c1, c0 = R.base(spec)
    for n, rot, idx in R.populations(spec, sizes=(1, 65)):
        for with_sec, want in ((True, c1[idx]), (False, c0[idx])):
            W = R.table(spec, idx)
            gc, gn, _ = K.run_fixpoint(spec, W, 0, EPS, with_sec=with_sec)
            assert np.array_equal(gc.numpy(), want) and not gn.any()


@pytest.mark.parametrize("spec", R.PREIMAGE, ids=R.sid)
def test_preimage_rows(spec):
    """the stored rows: not constant, other at the start, fix_sec after one self-application (the
    constant -a row), the +a fixpoint after two; the host engine agrees"""
    u = R.preimage(spec)[None]
    assert u.dtype == np.float32 and np.ptp(u) > 0.1
    f = O.apply(spec, u, u)
    assert np.max(np.abs(f + R.agg_a(spec))) < 1e-6
    assert O.classify(spec, u, R.EPS).tolist() == [O.C_OTHER]
    for steps, want in ((1, (1, O.C_FIX_SEC)), (5, (2, O.C_FIX_OTHER))):
        _, ns, cls = O.run_fixpoint(spec, u, steps, R.EPS)
        assert (int(ns[0]), int(cls[0])) == want
        W = torch.zeros(1, spec.PP)
        W[:, :spec.P] = torch.from_numpy(u)
        gc, gn, _ = K.run_fixpoint(spec, W, steps, EPS)
        assert (int(gn[0]), int(gc[0])) == want


def test_preimage_search_is_reproducible():
    """the search that found the stored rows (fixed seed, fixed iteration count) finds such a row again"""
    spec = R.PREIMAGE[0]
    u = R.solve_preimage(spec)[None]
    assert np.max(np.abs(O.apply(spec, u, u) + R.agg_a(spec))) < 1e-6
    assert O.run_fixpoint(spec, u, 1, R.EPS)[2].tolist() == [O.C_FIX_SEC]


# (the big aggregating nets have no scheduled reference-order generation on the host)
HOST_SOUPS = [(s, o) for s in (R.LANE[0], R.LANE[2], R.LANE[4], R.GENERIC[0], R.RNN_WAVE[0], R.BIG[0])
              for o in ("synchronous", "sequential") if not (o == "sequential" and s == R.BIG[0])]


@pytest.mark.parametrize("spec,order", HOST_SOUPS, ids=[f"{R.sid(s)}-{o}" for s, o in HOST_SOUPS])
def test_host_static_soup_census(spec, order):
    """a soup in which nothing happens reports the oracle's histogram of the constructed rows every
    generation: the fused census of the host generation and the close of the reference order"""
    R.check_static_soup(spec, "cpu", order=order)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_host_classify_16_bit_tables(dtype):
    """the rows that are exact in the storage format keep their class in a 16-bit table"""
    spec = R.LANE[0]
    rows = R.lowp_rows(spec, dtype)
    _, _, c1, c0 = R.base(spec)
    assert sum(R.histogram(c1[rows]) > 0) == 5
    for n, rot, idx in R.populations(spec, sizes=(65,), rows=rows):
        W = R.table(spec, idx, dtype=dtype)
        for with_sec, want in ((True, c1[idx]), (False, c0[idx])):
            cls, counts = K.classify(spec, W, EPS, with_sec=with_sec)
            assert np.array_equal(cls.numpy(), want) and np.array_equal(counts.numpy(), R.histogram(want))
