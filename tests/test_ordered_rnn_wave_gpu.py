"""Reference-order generations of the wide Recurrent runtime shapes on a wave per turn
(csrc/srnn_generic.hip k_gord_run_rnn: one wave per workgroup and index position, rw_forward /
rw_train_epoch on LDS row vectors, k_gord_run_ww's schedule with one turn per wave):

1. which form an engine takes, and that the knob (SRNN_KNOB_ORD_WAVE) turns the wave run off;
2. wave run == lane run on the same device, bitwise: the <8,2> instantiation (P = 209 > 64: the
   strided loops wrap), the runtime-shape <0,0> one (RNN(12,2)) and depth 3; fp32 and bf16 tables;
   continuations (levels >= 3), stored attack outputs and respawns (the lane-0 orthogonal init) occur;
3. every turn attacks and learns (SRC_SELF / SRC_ATK teachers, at == k), down to one particle;
4. a generation == the host serial loop (SequentialSoupEngine), respawn off (a newborn's orthogonal
   init goes through the device's libm and is not bitwise the host's);
5. graph chunks == eager; 6. the recorded pre-respawn rows; 7. serial == batched finish.

With the engine's own initial rows every row of these nets diverges under HOT's two epochs of SGD
(each generation respawns the whole population, no loss is finite), so beside those cases the same
comparisons run from the initial rows scaled by 0.5 (HALF), where every row and nearly every loss
stays finite and a few rows per generation fall to zero: there the bits compared are arithmetic.

RNN(16,2) and RNN(32,2) are not tested against a lane twin (their lane turn is too slow for a
test); bench/ordered_shapes.py selects and times them."""
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.config import ExecConfig
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.seq_soup import SequentialSoupEngine
from self_replicating_neural_networks_amd.soup_engine import SoupEngine

pytestmark = pytest.mark.gpu

HOT = dict(attacking_rate=0.3, learn_from_rate=0.3, train=2, learn_from_severity=2, remove_divergent=True,
           remove_zero=True, epsilon=1e-4)
RNN82 = ArchSpec.recurrent(8, 2)
SCALES = pytest.mark.parametrize("scale", [1.0, 0.5], ids=["init", "half"])


def _start_rows(spec, n, params, seed, scale, **kw):
    """the engine's own initial rows of this seed, scaled (None: unscaled, the engine draws them itself)"""
    if scale == 1.0:
        return None
    e = SoupEngine(spec, n, params, device="cuda", seed=seed, order="sequential", **kw)
    return e.local_rows()[:, :spec.P].float().cpu() * scale


def _all_finite(e, spec):
    return bool(torch.isfinite(e.local_rows()[:, :spec.P].float()).all())


def _bits(t):
    """the stored bit patterns (16-bit words of a bf16 / fp16 table, else 32-bit)"""
    return t.cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def canon(t):
    """Bit pattern of a tensor with every NaN mapped to one value (NaN payloads are not a contract)."""
    t = torch.nan_to_num(t.float().cpu(), 7.0, 9.0, -9.0).contiguous()
    return t.view(torch.int32)


class _ord_wave:
    """the process-global SRNN_KNOB_ORD_WAVE around one engine's calls"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib.set_knob("ord_wave", 1 if self.on else 0)

    def __exit__(self, *exc):
        _lib.set_knob("ord_wave", -1)


def _same_engines(a: SoupEngine, b: SoupEngine, P: int):
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.local_rows()[:, :P]), _bits(b.local_rows()[:, :P]))
    assert torch.equal(a.uid, b.uid) and int(a.next_uid[0]) == int(b.next_uid[0])
    assert torch.equal(a.action, b.action) and torch.equal(a.counterpart, b.counterpart)
    assert torch.equal(a.respawn, b.respawn)
    assert torch.equal(_bits(a.loss), _bits(b.loss))
    assert a.last_census() == b.last_census()
    assert a.ordered_levels()["error"] == 0 and b.ordered_levels()["error"] == 0


def _twins(spec, n, params, seed, scale=1.0, **kw):
    """a wave-run engine and a lane-run engine from the same rows"""
    rows0 = _start_rows(spec, n, params, seed, scale, **kw)
    kw = dict(dict(device="cuda", seed=seed, order="sequential"), **kw)
    with _ord_wave(True):
        w = SoupEngine(spec, n, params, weights=rows0, **kw)
        assert w._ord_generic and w.ordered_run_form() == "wave"
    with _ord_wave(False):
        l = SoupEngine(spec, n, params, weights=w.local_rows()[:, :spec.P].float().cpu(), **kw)
        assert l.ordered_run_form() == "lane"
    assert torch.equal(_bits(w.local_rows()), _bits(l.local_rows()))
    w.stats = l.stats = True
    return w, l


def _evolve_both(w, l, spec, steps):
    """evolve the twins by each of `steps`, compare after each; -> deepest level, stored attacks, respawns"""
    deep = stored = dead = 0
    for k in steps:
        with _ord_wave(True):
            w.evolve(k)
            torch.cuda.synchronize()
        with _ord_wave(False):
            l.evolve(k)
        _same_engines(w, l, spec.P)
        lv = w.ordered_levels()
        deep = max(deep, lv["max_level"])
        stored += lv["stored_attacks"]
        dead += int((w.respawn != 0).sum())
        print(f"{spec} after {k} more: {lv}, respawns {int((w.respawn != 0).sum())}")
    return deep, stored, dead


# ---------------------------------------------------------------- 1. form selection
def test_an_engine_takes_the_wave_run_and_the_knob_turns_it_off():
    assert _lib.get_knob("ord_wave") == -1
    for on, form in ((True, "wave"), (False, "lane")):
        try:
            with _ord_wave(on):
                assert _lib.ord_run_form(RNN82, dev=True) == form
                e = SoupEngine(RNN82, 70, HOT, device="cuda", seed=2, order="sequential",
                               execution=ExecConfig(ord_wave=on))
                assert e._ord_generic and e.ordered_run_form() == form
                e.evolve(1)
                torch.cuda.synchronize()
                assert e.ordered_levels()["error"] == 0
        finally:
            _lib.set_knob("ord_wave", -1)


# ---------------------------------------------------------------- 2. wave run == lane run
@SCALES
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("spec,n,steps", [(RNN82, 203, (1, 2, 2)), (ArchSpec.recurrent(12, 2), 131, (1, 2)),
                                          (ArchSpec.recurrent(8, 3), 131, (1, 2))],
                         ids=["rnn82-spec", "rnn122-runtime", "rnn83-spec"])
def test_wave_run_equals_lane_run(spec, n, steps, dtype, scale):
    """rows' bit patterns, uid, next_uid, action, counterpart, respawn, loss bits and census after 1, 2
    and 2 more generations (RNN(12,2) and RNN(8,3): 1 and 2 -- their lane-run twin takes 0.35 s per
    dependency level, 1.7 s per generation); continuations, a stored attack output and a respawn occur
    (seed 7).  From the half-scale rows every row stays finite."""
    try:
        w, l = _twins(spec, n, HOT, 7, scale, dtype=dtype)
        deep, stored, dead = _evolve_both(w, l, spec, steps)
        assert sum(w.last_census().values()) == n
        assert deep >= 3
        assert stored > 0 and dead > 0
        if scale != 1.0:
            assert _all_finite(w, spec) and int(torch.isfinite(w.loss).sum()) > n // 2
    finally:
        _lib.set_knob("ord_wave", -1)


# ---------------------------------------------------------------- 3. every turn attacks and learns
@SCALES
@pytest.mark.parametrize("n", [67, 5, 1])
def test_every_turn_attacks_and_learns(n, scale):
    try:
        w, l = _twins(RNN82, n, dict(HOT, attacking_rate=1.0, learn_from_rate=1.0), 5, scale)
        deep, stored, _ = _evolve_both(w, l, RNN82, (1, 2))
        assert n == 1 or (stored > 0 and deep >= 3)
    finally:
        _lib.set_knob("ord_wave", -1)


# ---------------------------------------------------------------- 4. the host serial loop
@SCALES
def test_wave_run_is_the_host_serial_loop(scale):
    """rows (NaNs canonicalised), action, counterpart, uid and loss bits == the host serial loop over
    three generations, respawn off.  From the engine's own rows every row is non-finite after the first
    generation; from the half-scale rows every row stays finite."""
    spec, n = RNN82, 203
    params = dict(HOT, remove_divergent=False, remove_zero=False)
    o = SoupEngine(spec, n, params, device="cuda", seed=11, order="sequential",
                   weights=_start_rows(spec, n, params, 11, scale))
    assert o._ord_generic and o.ordered_run_form() == "wave"
    o.stats = True
    s = SequentialSoupEngine(spec, n, params, seed=11, weights=o.local_rows()[:, :spec.P].float().cpu())
    for g in range(3):
        o.evolve(1)
        s.evolve(1)
        torch.cuda.synchronize()
        lv = o.ordered_levels()
        assert lv["error"] == 0, g
        assert torch.equal(o.action.cpu(), s.action.cpu()), g
        assert torch.equal(o.counterpart.cpu(), s.counterpart.cpu()), g
        assert torch.equal(o.uid.cpu(), s.uid.cpu()), g
        bad = int((canon(o.local_rows()[:, :spec.P]) != canon(s.W[:, :spec.P])).any(dim=1).sum())
        print(f"{spec} generation {g}: {lv}; rows that differ from the host loop {bad}/{n}")
        assert bad == 0, g
        assert torch.equal(_bits(o.loss), _bits(s.loss)), g
    assert scale == 1.0 or (_all_finite(o, spec) and bool(torch.isfinite(o.loss).all()))


# ---------------------------------------------------------------- 5. graph chunks
@SCALES
def test_graph_chunks_of_the_wave_run_equal_eager(scale):
    spec, n = RNN82, 131
    g = SoupEngine(spec, n, HOT, device="cuda", seed=3, order="sequential", execution=ExecConfig(graph_chunks=(2,)),
                   weights=_start_rows(spec, n, HOT, 3, scale))
    e = SoupEngine(spec, n, HOT, device="cuda", seed=3, order="sequential",
                   weights=g.local_rows()[:, :spec.P].float().cpu())
    assert g.ordered_run_form() == e.ordered_run_form() == "wave"
    g.stats = e.stats = True
    assert g.capture(warmup=1)  # (one generation)
    e.evolve(1)
    _same_engines(g, e, spec.P)
    g.evolve(2)
    e.evolve(2)
    _same_engines(g, e, spec.P)
    g.release_graphs()


# ---------------------------------------------------------------- 6. recording
class _Rows:
    """a recorder that keeps each generation's pre-respawn rows"""

    def __init__(self):
        self.rows = []

    def on_evolved(self, engine, rows=None, old_uid=None, ordered=False):
        assert ordered and rows is not None
        torch.cuda.synchronize()
        self.rows.append(rows.clone())

    def on_generation_end(self, engine, t, slot_uid):
        pass


@SCALES
def test_recorded_rows_of_wave_run_and_lane_run_are_equal(scale):
    spec, n = RNN82, 131
    recs = []
    try:
        rows0 = _start_rows(spec, n, HOT, 7, scale)
        for on in (True, False):
            with _ord_wave(on):
                e = SoupEngine(spec, n, HOT, device="cuda", seed=7, order="sequential", weights=rows0)
                assert e.ordered_run_form() == ("wave" if on else "lane")
                if rows0 is None:
                    rows0 = e.local_rows()[:, :spec.P].float().cpu()
                e.recorder = _Rows()
                e.evolve(2, record=True)
                torch.cuda.synchronize()
                assert e.ordered_levels()["error"] == 0
                recs.append((e.recorder.rows, e.local_rows().clone(), e.respawn.clone()))
    finally:
        _lib.set_knob("ord_wave", -1)
    (ra, fa, sa), (rb, fb, sb) = recs
    assert len(ra) == len(rb) == 2
    for x, y in zip(ra, rb):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(_bits(fa), _bits(fb)) and torch.equal(sa, sb)
    # a respawned row was recorded as it was before its re-initialisation
    dead = (sa != 0).nonzero().flatten()
    assert len(dead) > 0
    assert not torch.equal(canon(ra[-1][dead, :spec.P]), canon(fa[dead, :spec.P]))


# ---------------------------------------------------------------- 7. finish modes
def test_wave_run_serial_and_batched_finish_agree():
    spec, n = RNN82, 203
    es = [SoupEngine(spec, n, HOT, device="cuda", seed=4, order="sequential", execution=ExecConfig(finish_mode=fm))
          for fm in ("serial", "batch")]
    assert [e.finish_mode for e in es] == ["serial", "batch"]
    for e in es:
        assert e.ordered_run_form() == "wave"
        e.stats = True
        e.evolve(2)
    _same_engines(es[0], es[1], spec.P)
    assert torch.equal(es[0].counts, es[1].counts)
    assert es[0].last_census() == es[0].count()
