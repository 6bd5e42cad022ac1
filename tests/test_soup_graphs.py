"""Graph validation (soup_graphs._validate_replay) on the host, where capture() returns False and
nothing else runs its save / restore / compare: a replay that is the eager generations passes, one
that is a generation short or leaves one flipped uid bit fails, and either way the engine's host
and device state come back -- a later evolve is bitwise a twin's that never validated."""
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from self_replicating_neural_networks_amd import soup_graphs
from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.config import ExecConfig
from self_replicating_neural_networks_amd.parallel.dist import Dist
from self_replicating_neural_networks_amd.seq_soup import SequentialSoupEngine
from self_replicating_neural_networks_amd.soup_engine import SoupEngine

from test_dist_gloo import _free_port
from test_ordered_soup import HOT, _same

N = 192  # three 64-row blocks
WW22, WW33 = ArchSpec.weightwise(2, 2), ArchSpec.weightwise(3, 3)
CASES = {"ww22-sync": (WW22, "synchronous", None), "ww33-sync": (WW33, "synchronous", None),
         "ww22-seq-stream": (WW22, "sequential", "stream"), "ww22-seq-off": (WW22, "sequential", "off"),
         "ww33-seq": (WW33, "sequential", None)}


def _engine(case, **kw):
    """The case's engine after one generation."""
    spec, order, pipe = CASES[case]
    ex = ExecConfig(ord_pipeline=pipe) if pipe else None
    e = SoupEngine(spec, N, HOT, device="cpu", seed=5, order=order, execution=ex, **kw)
    e.stats = True
    return e.evolve(1)


def _gens(e, k, flip=False):
    """A "replay" that runs k eager generations (and then flips one bit of one uid)."""
    def replay():
        for _ in range(k):
            e._generation()
        e._join_side()
        if flip:
            e.uid[0] ^= 1
    return replay


def _bytes(e):
    return [t.contiguous().view(torch.uint8).clone() for t in (e.local_rows(), e.uid, e.next_uid, e.counts, e.census)]


_TWINS = {}


def _twin(case):
    """Rows, uids and census of the case's engine after evolve(3), never validated (computed once)."""
    if case not in _TWINS:
        _TWINS[case] = _bytes(_engine(case).evolve(3))
    return _TWINS[case]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("replay,want", [("same", True), ("short", False), ("flip", False)])
def test_validation_compares_and_restores(case, replay, want):
    e = _engine(case)
    assert e.fused == (CASES[case][0] is WW22 or CASES[case][1] == "sequential")
    host0 = e._host_state()
    dev0 = [t.clone() for t in e._state()]
    f = _gens(e, 2 if replay == "short" else 3, flip=replay == "flip")
    assert soup_graphs._validate_replay(e, f, 3) is want
    assert e._host_state() == host0
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(e._state(), dev0))
    e.evolve(3)
    assert e.time == 4
    assert all(torch.equal(a, b) for a, b in zip(_bytes(e), _twin(case)))


def test_host_state_has_every_field_on_every_engine_kind():
    """the batched finish's counters and the sharded exchange's _primed exist on engines without either"""
    assert {"_p", "time", "_pending", "_lists_ready", "_pending_fin", "_census_due", "_census_log_rows",
            "_fin_flags", "_primed"} == set(SoupEngine.HOST_STATE)
    for case in ("ww22-sync", "ww33-seq"):
        e = _engine(case)
        st = e._host_state()
        assert st == tuple(getattr(e, k) for k in SoupEngine.HOST_STATE)
        assert (e._pending_fin, e._fin_flags, e._primed) == (0, 0, False)
        e.evolve(1)
        assert e._host_state() != st
        e._set_host_state(st)
        assert e._host_state() == st


def test_state_raises_on_a_name_the_engine_never_initialises(monkeypatch):
    e = _engine("ww22-sync")
    assert set(SoupEngine.COMPARED_STATE) <= set(SoupEngine.DEVICE_STATE)
    monkeypatch.setattr(SoupEngine, "DEVICE_STATE", SoupEngine.DEVICE_STATE + ("_no_such_buffer",))
    with pytest.raises(AttributeError, match="_no_such_buffer"):
        e._state()


def _worker(rank, world, port, kind):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        order = "sequential" if kind == "sequential" else "synchronous"
        e = SoupEngine(WW22, N, HOT, device="cpu", seed=5, dist=Dist(rank, world, 0, None), order=order)
        assert e.x2 == (kind == "alltoall")
        e.stats = True
        e.evolve(1)
        host0 = e._host_state()
        dev0 = [t.clone() for t in e._state()]
        assert soup_graphs._validate_replay(e, _gens(e, 3), 3) is True
        assert e._host_state() == host0
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(e._state(), dev0))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["alltoall", "sequential"])
def test_validation_on_two_ranks(kind):
    mp.start_processes(_worker, args=(2, _free_port(), kind), nprocs=2, start_method="spawn", join=True)


@pytest.mark.gpu
def test_a_short_replay_of_a_two_graph_chunk_is_refused():
    """device, reference order, default ExecConfig: the captured 4-generation chunk with a side graph,
    validated against a replay one generation short, is refused; the engine then evolves bitwise
    the serial loop (state restored, graphs intact)"""
    o = SoupEngine(WW22, N, HOT, device="cuda", seed=5, order="sequential")
    s = SequentialSoupEngine(WW22, N, HOT, seed=5, device="cuda", weights=o.local_rows()[:, :WW22.P].cpu())
    assert o.capture(warmup=1)
    s.evolve(1)
    ch = next(c for c in o._chunks if c.side is not None and c.gens == 4 and c.parity == o._p)
    host0 = o._host_state()

    def short():
        for _ in range(ch.gens - 1):
            o._graphs[o._p].replay()
            o._p = 1 - o._p

    assert soup_graphs._validate_replay(o, short, ch.gens, chunk=True, ring=o.finish_mode == "batch") is False
    assert o._host_state() == host0
    o.evolve(4)
    s.evolve(4)
    _same(o, s, WW22.P)
    assert o.ordered_levels()["error"] == 0
    o.release_graphs()
