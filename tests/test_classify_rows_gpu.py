"""Every device classifier on the constructed rows of tests/classify_rows.py, on every route, with 0
mismatches against ``oracle.core.classify`` / ``run_fixpoint`` allowed.  Each test forces its route
and asserts that it is the one in force.  The fix_sec branch of each implementation is reached
with a POSITIVE result (class 3 reported for the negated identities, the (-4, 0.25) rows, the
perturbed negated identities, the constant -a rows, or the state after the preimages' first step) by

  classify_w          k_classify_count, k_op<OP_RUN_FIXPOINT>: test_lane_templates (SRNN_FIX_GROUP=0);
                      k_soup_gen / k_soup_evolve: test_static_soup_census[ww-2-2-lanes1 / -unfused /
                      -graph]; k_ord_close: test_static_reference_order_census[ww-2-2]
  k_fix_group         test_fix_group (WW(2, 1) and WW(1, 1) END in fix_sec after 7 steps)
  pair::classify      test_static_soup_census[ww-2-2-lanes2] (k_soup_gen2)
  g_classify_w        test_runtime_shapes (k_generic), test_static_soup_census[ww-3-3 / rnn-8-2 /
                      rnn-3-2], test_static_reference_order_census[ww-3-3 / rnn-8-2] (k_ord_close<GOrdPol>)
  rw_classify         test_rnn_wave (k_rnn_wave by run_fixpoint: OP_CLASSIFY of these shapes is
                      k_generic's); RNN(8, 3) ends in fix_sec after 7 steps
  wide_classify       test_wide (k_wide, both MFMA column tiles of WW(32, 2): units 0 and 31)
  sclassify           test_big_nets[row] (k_big_rows by classify, k_big_fix1_row by run_fixpoint of
                      rows that take no step), test_static_soup_census[agg-8-2]
  bclassify           test_static_soup_census[agg-8-2-shuf] (k_big_rows<SHUF> takes the census of the
                      generations of k_big_soup_evolve)
  classify_lds        test_big_nets[wave] (SRNN_BIG_WAVE=1: k_big<OP_CLASSIFY>, k_big_fix1)
  the branch of k_big_fix2
                      test_big_preimages, both settings (steps = 1: fix_sec, the state after the first
                      step; k_big_fix2 classifies every row that took a step)

Each line was confirmed once by breaking the second-order comparison of that classifier in a build made
for the purpose and not kept: the tests named fail (so does a test that reads count() or K.classify
beside a census, when that kernel's classifier is the broken one).

Not reachable from Python, left out: ``lclassify`` -- k_big_row<OP_CLASSIFY> is launched only when
SRNN_BIG_WAVE=1 selects the wave kernels and the row kernels at once, which big_run never does
(OP_CLASSIFY of the big nets is k_big_rows or k_big) -- and ``classify_state``, whose only caller
k_big<OP_RUN_FIXPOINT> is never launched (run_fixpoint of the big nets is k_big_fix1 / 2 / 3 on
both settings; the state after a step is classified by k_big_fix2).  The odd-depth shapes
Aggregating(4, 4, 3) and (4, 10, 3) reach the branch with a negative result only: no fix_sec row
exists for them (tests/classify_rows.py)."""
import numpy as np
import pytest
import torch

import classify_rows as R
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.oracle import core as O

pytestmark = pytest.mark.gpu
EPS = float(R.EPS)
F32 = _lib.DTYPE_FP32


def _names(spec, idx, got, want):
    bad = np.nonzero(got != want)[0]
    return [(int(i), R.base(spec)[0][idx[i]], int(got[i]), int(want[i])) for i in bad[:8]]


def check_classify(spec, dev, dtype=torch.float32, rows=None, sizes=R.SIZES):
    """K.classify on every population: classes, histogram, both settings of the second-order test"""
    _, _, c1, c0 = R.base(spec)
    for n, rot, idx in R.populations(spec, sizes, rows):
        W = R.table(spec, idx, dev, dtype)
        for with_sec, want in ((True, c1[idx]), (False, c0[idx])):
            cls, counts = K.classify(spec, W, EPS, with_sec=with_sec)
            got = cls.cpu().numpy()
            assert np.array_equal(got, want), (n, rot, with_sec, _names(spec, idx, got, want))
            assert np.array_equal(counts.cpu().numpy(), R.histogram(want)), (n, rot, with_sec)
        if n > 1 and rows is None:
            assert sum(R.histogram(c1[idx]) > 0) == R.n_classes(spec)


def check_run(spec, dev, dtype=torch.float32, sizes=(65, 257)):
    """K.run_fixpoint: 7 steps with and without the early exit (classes and step counts), and 0
    steps -- the classifier of the run alone -- on every row"""
    for early in (True, False):
        rr = R.run_rows(spec, early)
        where = {int(r): k for k, r in enumerate(rr)}
        _, ns, cls = R.base_run(spec, 7, early)
        for n, rot, idx in R.populations(spec, sizes, rr):
            sel = np.array([where[int(i)] for i in idx])
            W = R.table(spec, idx, dev, dtype)
            gc, gn, _ = K.run_fixpoint(spec, W, 7, EPS, early_exit=early)
            got = gc.cpu().numpy()
            assert np.array_equal(got, cls[sel]), (n, rot, early, _names(spec, idx, got, cls[sel]))
            assert np.array_equal(gn.cpu().numpy(), ns[sel]), (n, rot, early)
    _, _, c1, c0 = R.base(spec)
    for n, rot, idx in R.populations(spec, sizes):
        for with_sec, want in ((True, c1[idx]), (False, c0[idx])):
            W = R.table(spec, idx, dev, dtype)
            gc, gn, _ = K.run_fixpoint(spec, W, 0, EPS, with_sec=with_sec)
            got = gc.cpu().numpy()
            assert np.array_equal(got, want), (n, rot, with_sec, _names(spec, idx, got, want))
            assert not gn.any()


def ends_in_fix_sec(spec):
    """the period-2 rows (an even number of kernels on the path) keep run_fixpoint going for all 7
    steps and end as fix_sec"""
    _, ns, cls = R.base_run(spec, 7, True)
    sec = cls == O.C_FIX_SEC
    return sec.any() and (ns[sec] == 7).all()


# ------------------------------------------------------------------------------ 1. lane templates
@pytest.mark.parametrize("spec", R.LANE, ids=R.sid)
def test_lane_templates(cuda, spec, monkeypatch):
    """k_classify_count and k_op<OP_RUN_FIXPOINT> (classify_w)"""
    monkeypatch.setenv("SRNN_FIX_GROUP", "0")
    assert _lib.get_knob("fix_group") == 0
    for op in (_lib.OP_CLASSIFY, _lib.OP_RUN_FIXPOINT):
        assert not _lib.is_generic(spec, op, F32)
    assert not K.is_wave_per_particle(spec)
    check_classify(spec, cuda)
    check_run(spec, cuda)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_lane_templates_16_bit_tables(cuda, dtype, monkeypatch):
    """WW(2, 2) with 16-bit tables: the rows that are exact in the storage format keep their class"""
    spec = R.LANE[0]
    monkeypatch.setenv("SRNN_FIX_GROUP", "0")
    assert not _lib.is_generic(spec, _lib.OP_CLASSIFY, K.dtype_code(dtype))
    rows = R.lowp_rows(spec, dtype)
    assert sum(R.histogram(R.base(spec)[2][rows]) > 0) == 5
    check_classify(spec, cuda, dtype, rows=rows)
    W = R.table(spec, R.population(spec, 65, 3, rows), cuda, dtype)
    want = R.base(spec)[2][R.population(spec, 65, 3, rows)]
    gc, gn, _ = K.run_fixpoint(spec, W, 0, EPS)
    assert np.array_equal(gc.cpu().numpy(), want)


# ------------------------------------------------------------------------------ 2. k_fix_group
@pytest.mark.parametrize("spec", R.FIX_GROUP, ids=R.sid)
def test_fix_group(cuda, spec, monkeypatch):
    """the open-coded classifier of k_fix_group (16 lanes per particle)"""
    monkeypatch.setenv("SRNN_FIX_GROUP", "1")
    assert _lib.get_knob("fix_group") == 1 and spec.kind == "weightwise" and spec.P <= 16
    assert not _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT, F32)
    assert ends_in_fix_sec(spec) == (spec.depth == 1)
    check_run(spec, cuda, sizes=R.SIZES)


# ------------------------------------------------------------------------------ 3. k_generic
@pytest.mark.parametrize("spec", R.GENERIC, ids=R.sid)
def test_runtime_shapes(cuda, spec):
    """k_generic (g_classify_w)"""
    for op in (_lib.OP_CLASSIFY, _lib.OP_RUN_FIXPOINT):
        assert _lib.is_generic(spec, op, F32)
    assert spec.kind != "recurrent" or spec.width < 8  # (not the wave kernels of the wide Recurrent nets)
    check_classify(spec, cuda)
    check_run(spec, cuda)


@pytest.mark.parametrize("spec", [R.LANE[0], R.LANE[2]], ids=R.sid)
def test_template_shapes_on_the_runtime_engine(cuda, spec, monkeypatch):
    monkeypatch.setenv("SRNN_FORCE_GENERIC", "1")
    for op in (_lib.OP_CLASSIFY, _lib.OP_RUN_FIXPOINT):
        assert _lib.is_generic(spec, op, F32)
    check_classify(spec, cuda)
    check_run(spec, cuda)


# ------------------------------------------------------------------------------ 4. k_rnn_wave
@pytest.mark.parametrize("spec", R.RNN_WAVE, ids=R.sid)
def test_rnn_wave(cuda, spec):
    """rw_classify: run_fixpoint of the wide Recurrent nets, a wave per particle, units 0 and W - 1"""
    assert _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT, F32) and spec.width >= 8
    assert _lib.get_knob("rnn_wave") != 0 and _lib.get_knob("force_generic") != 1
    assert {"negid0", f"negid{spec.width - 1}"} <= set(R.base(spec)[0])
    assert ends_in_fix_sec(spec) == (spec.depth == 3)
    check_run(spec, cuda)
    check_classify(spec, cuda)  # (k_generic)


# ------------------------------------------------------------------------------ 5. k_wide
@pytest.mark.parametrize("spec", R.WIDE, ids=R.sid)
def test_wide(cuda, spec):
    """wide_classify on the MFMA path; unit W - 1 of WW(32, 2) lies in the second 16-column tile"""
    assert K.is_wave_per_particle(spec)
    for op in (_lib.OP_CLASSIFY, _lib.OP_RUN_FIXPOINT):
        assert not _lib.is_generic(spec, op, F32)
    assert {"negid0", f"negid{spec.width - 1}"} <= set(R.base(spec)[0])
    assert ends_in_fix_sec(spec) == (spec.depth == 3)
    check_classify(spec, cuda)
    check_run(spec, cuda)


def test_wide_period_two_trajectory(cuda):
    """WW(16, 3), negated identities through units 0 and 15: 7 early-exit steps never exit, end in
    fix_sec, and the recorded rows alternate w, -w (exact values; the sign of a zero is free)"""
    spec = R.WIDE[1]
    assert K.is_wave_per_particle(spec) and not _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT, F32)
    names = R.base(spec)[0]
    idx = np.array([names.index("negid0"), names.index("negid15"), names.index("pow2_0"), names.index("pow2_15")] * 17)
    W = R.table(spec, idx, cuda)
    w0 = W.clone()
    cls, ns, traj = K.run_fixpoint(spec, W, 7, EPS, early_exit=True, record=True)
    assert cls.tolist() == [O.C_FIX_SEC] * len(idx) and ns.tolist() == [7] * len(idx)
    assert traj.shape == (8, len(idx), spec.PP)
    for s in range(8):
        assert torch.equal(traj[s], w0 if s % 2 == 0 else -w0), s
    assert torch.equal(W, -w0)


# ------------------------------------------------------------------------------ 6. big aggregating nets
@pytest.mark.parametrize("mode", ["row", "wave"])
@pytest.mark.parametrize("spec", R.BIG, ids=R.sid)
def test_big_nets(cuda, spec, mode, monkeypatch):
    """K.classify on the row kernels (sclassify) and with SRNN_BIG_WAVE=1 (classify_lds);
    run_fixpoint on the chunk-state kernels of either setting"""
    if mode == "wave":
        monkeypatch.setenv("SRNN_BIG_WAVE", "1")
    else:
        monkeypatch.delenv("SRNN_BIG_WAVE", raising=False)
    assert (_lib.get_knob("big_wave") == 1) == (mode == "wave")
    for op in (_lib.OP_CLASSIFY, _lib.OP_RUN_FIXPOINT):
        assert not _lib.is_generic(spec, op, F32)
    assert K.needs_chunk_state_temp(spec, torch.zeros(1, spec.PP, device=cuda))
    check_classify(spec, cuda)
    check_run(spec, cuda)


@pytest.mark.parametrize("mode", ["row", "wave"])
@pytest.mark.parametrize("spec", R.PREIMAGE, ids=R.sid)
def test_big_preimages(cuda, spec, mode, monkeypatch):
    """the chunk-state kernels (k_big_fix1 / _row -> k_big_fix2 -> k_big_fix3 / _row) classify the state
    AFTER the first step, in k_big_fix2: the preimages of the constant -a row are fix_sec at
    steps = 1 and the +a fixpoint at steps = 5"""
    if mode == "wave":
        monkeypatch.setenv("SRNN_BIG_WAVE", "1")
    else:
        monkeypatch.delenv("SRNN_BIG_WAVE", raising=False)
    assert (_lib.get_knob("big_wave") == 1) == (mode == "wave")
    assert not _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT, F32)
    names = R.base(spec)[0]
    pre, neg, pos, five = (names.index(k) for k in ("preimage", "const-a", "const+a", "zero+5"))
    for n in (1, 65, 257):
        idx = np.array(([pre, five, pre, neg, pos] * 52)[:n])
        rows = R.base(spec)[1][idx]
        for steps in (1, 5):
            for with_sec in (True, False):
                _, ns, cls = O.run_fixpoint(spec, rows, steps, R.EPS, True, with_sec)
                if with_sec:
                    assert (int(ns[0]), int(cls[0])) == ((1, O.C_FIX_SEC) if steps == 1 else (2, O.C_FIX_OTHER))
                W = R.table(spec, idx, cuda)
                assert K.needs_chunk_state_temp(spec, W)
                gc, gn, _ = K.run_fixpoint(spec, W, steps, EPS, early_exit=True, with_sec=with_sec)
                assert np.array_equal(gc.cpu().numpy(), cls) and np.array_equal(gn.cpu().numpy(), ns), (n, steps)


# ------------------------------------------------------------------------------ 7. / 8. static soups
class _knob:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        if self.name:
            _lib.set_knob(self.name, self.value)
            assert _lib.get_knob(self.name) == self.value

    def __exit__(self, *exc):
        if self.name:
            _lib.set_knob(self.name, -1)


def _synchronous(generic):
    def route(e):
        assert e.order == "synchronous" and e.generic == generic
    return route


AGG82S = R.AGG(4, 8, 2, shuffler="random")
SOUPS = {
    # id: (spec, knob, value, fused, graph, generic engine)
    "ww-2-2-lanes1": (R.LANE[0], "soup_lanes", 1, None, False, False),
    "ww-2-2-lanes2": (R.LANE[0], "soup_lanes", 2, None, False, False),
    "ww-2-2-unfused": (R.LANE[0], "soup_lanes", 1, False, False, False),
    "ww-2-2-graph": (R.LANE[0], "soup_lanes", 1, None, True, False),
    "ww-3-3": (R.GENERIC[0], "ww_wave", 1, None, False, True),
    "rnn-8-2": (R.RNN_WAVE[0], "rnn_soup", 1, None, False, True),
    "agg-8-2": (R.BIG[0], None, 0, None, False, True),
    "agg-8-2-shuf": (AGG82S, None, 0, None, False, True),
    "agg-8-2-graph": (R.BIG[0], None, 0, None, True, True),
    "rnn-3-2": (R.GENERIC[2], None, 0, None, False, True),
}


@pytest.mark.parametrize("name", list(SOUPS))
def test_static_soup_census(cuda, name):
    """the census of the synchronous generation: fused into k_soup_gen / k_soup_gen2 (classify_w,
    pair::classify) or taken by the classify kernel of the shape after k_soup_evolve,
    k_ww_wave_soup, k_rnn_wave_soup, k_big_soup_evolve and the runtime-shape evolve"""
    spec, knob, value, fused, graph, generic = SOUPS[name]
    if spec.kind == "aggregating" and spec.P > 64:  # (the row kernels evolve, the engine's generation is unfused)
        assert not _lib.is_generic(spec, _lib.OP_SOUP_EVOLVE, F32) and not _lib.is_generic(spec, _lib.OP_CLASSIFY, F32)
    elif generic:
        assert _lib.is_generic(spec, _lib.OP_SOUP_EVOLVE, F32)
    else:
        assert not _lib.is_generic(spec, _lib.OP_SOUP_GEN, F32)
    with _knob(knob, value):
        R.check_static_soup(spec, cuda, fused=fused, graph=graph, route=_synchronous(generic))


ORDERED = {"ww-2-2": (R.LANE[0], "lane", False), "ww-3-3": (R.GENERIC[0], "wave", True),
           "rnn-8-2": (R.RNN_WAVE[0], "wave", True), "agg-8-2": (R.BIG[0], "lane", False)}


@pytest.mark.parametrize("name", list(ORDERED))
def test_static_reference_order_census(cuda, name):
    """the close of the reference-order generation packs the class counts into the block stats (fix_sec:
    the high half of word 2): lane run, group run, wave run and the big nets' run"""
    spec, form, generic = ORDERED[name]

    def route(e):
        assert e.ordered_run_form() == form and e._ord_generic == generic
        assert _lib.is_generic(spec, _lib.OP_SOUP_ORDERED, F32) == generic

    R.check_static_soup(spec, cuda, order="sequential", route=route)
