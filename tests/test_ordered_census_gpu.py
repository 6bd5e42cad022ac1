"""The device census of a reference-order soup against independent oracles, on every route it can
take (tests/test_ordered_census.py has the identities, the populations and the host matrix).

With ExecConfig.ord_census_side and the batched finish the close leaves the class counts of its block
stats to one of three later places (SRNN_F_ORD_CENSUS_LATER):

  side stream  k_ord_census beside the next generation: every generation but the last of an eager
               multi-generation evolve and of a one-graph chunk
  join         k_ord_census on the main stream: the last generation of every evolve call / chunk
  in-run       extra workgroups of the NEXT generation's k_ord_run (o_census_temp): every generation
               but the last of a two-graph chunk

``counts`` keeps the last generation of a finish launch only -- always a join census -- so the
side-stream and in-run censuses are read from the per-generation log (SoupEngine.census_log) and
compared with a twin engine stepped one generation at a time.  With the serial finish, the
in-kernel pipeline or no pipeline the close takes the census itself.  The oracles are count() (the
classify kernel on the final rows) and the device serial loop's count(), never another engine on
the same route."""
import pytest
import torch

from self_replicating_neural_networks_amd.config import ExecConfig
from test_ordered_census import IDS, SIZES, SPECS, check_census, population
from test_ordered_soup import _same

pytestmark = pytest.mark.gpu

# (ord_pipeline, ord_graph_sync, ord_census_side, finish_mode); sync / side only matter with the side stream
STREAM = [("stream", sync, side, fin) for sync in (True, False) for side in (True, False)
          for fin in ("batch", "serial")]
OTHER = [(pipe, True, True, fin) for pipe in ("kernel", "off") for fin in ("batch", "serial")]


def _cid(c):
    pipe, sync, side, fin = c
    if pipe != "stream":
        return f"{pipe}-{fin}"
    return f"stream-{'2g' if sync else '1g'}-side{int(side)}-{fin}"


def _exec(pipe, sync, side, fin, **kw):
    return ExecConfig(ord_pipeline=pipe, ord_graph_sync=sync, ord_census_side=side, finish_mode=fin,
                      graph_chunks=(4, 2), **kw)


def _census_routes(kind, n, cfg, min_classes):
    pipe, sync, side, fin = cfg
    # eager, one generation per call: the census of each by the close or at the join
    o, s = population(kind, n, device="cuda", execution=_exec(*cfg))
    assert o._ord_mode == pipe and o.finish_mode == fin
    assert o._ord_census_side == (pipe == "stream" and side)
    for _ in range(6):
        uid0 = int(o.next_uid[0])
        o.evolve(1)
        s.evolve(1)
        _same(o, s, o.spec.P)
        check_census(o, s, uid_before=uid0, min_classes=min_classes)
    assert o.ordered_levels()["error"] == 0
    # graphed: chunks of 4 and 2 generations, single-generation graphs between them
    o, s = population(kind, n, device="cuda", execution=_exec(*cfg))
    uid0 = int(o.next_uid[0])
    assert o.capture(warmup=1)
    s.evolve(1)  # capture runs one warmup generation eagerly
    # (every chunk validated bitwise against eager generations; the two-graph form kept where asked for)
    assert any(c[3] is not None for c in o._chunks) == (pipe == "stream" and sync)
    assert sorted({c[2] for c in o._chunks}) == [2, 4]
    _same(o, s, o.spec.P)
    check_census(o, s, uid_before=uid0, min_classes=min_classes)
    for k in (2, 4, 1, 4, 3):
        o.evolve(k)
        s.evolve(k)
        _same(o, s, o.spec.P)
        check_census(o, s, min_classes=min_classes)
    assert o.ordered_levels()["error"] == 0
    o.release_graphs()


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
@pytest.mark.parametrize("cfg", STREAM + OTHER, ids=_cid)
def test_device_ordered_census_of_the_hot_soup(cfg, spec):
    """3000 particles (46 full blocks and one of 56 rows), respawns every generation: counts[0:5]
    and the ballots' counts[5] on every schedule, eager and in hipGraphs"""
    _census_routes(spec, 3000, cfg, 1)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cfg", STREAM, ids=_cid)
def test_device_ordered_census_of_the_seeded_population(cfg, n):
    """five non-empty classes (both halves of block-stat words 1 and 2, word 3) at one partial block,
    exactly one, two and a tail, and 47"""
    _census_routes("seeded", n, cfg, 5)


def test_device_ordered_census_without_second_order_fixpoints():
    """stats_with_sec = False against count(with_sec=False): the deferred census carries the flag"""
    o, s = population("seeded", 130, device="cuda", execution=_exec("stream", True, True, "batch"))
    o.stats_with_sec = False
    assert o.capture(warmup=1)
    s.evolve(1)
    assert any(c[3] is not None for c in o._chunks)
    for k in (1, 4, 3):
        o.evolve(k)
        s.evolve(k)
        got = check_census(o, s, with_sec=False, min_classes=4)
        sec = s.count(with_sec=True)  # the second-order fixpoints are there and are counted as other
        assert got["fix_sec"] == 0 < sec["fix_sec"] and got["other"] == sec["other"] + sec["fix_sec"]
    o.release_graphs()


def _twin_rows(kind, n, skip, gens):
    """[classes[5], respawns] of ``gens`` generations after ``skip``, from an engine without a census
    log stepped one generation at a time: count() on its rows and the advance of next_uid"""
    t, s = population(kind, n, device="cuda", execution=_exec("off", True, False, "batch"))
    t.evolve(skip)
    s.evolve(skip)
    rows = []
    for _ in range(gens):
        uid0 = int(t.next_uid[0])
        t.evolve(1)
        s.evolve(1)
        c = t.count()
        assert c == s.count()
        rows.append(list(c.values()) + [int(t.next_uid[0]) - uid0])
    _same(t, s, t.spec.P)
    return torch.tensor(rows, dtype=torch.int64), t


@pytest.mark.parametrize("kind", ["seeded", SPECS[0]], ids=["seeded", "hot"])
@pytest.mark.parametrize("side", [True, False], ids=["side1", "side0"])
@pytest.mark.parametrize("run", ["two-graph", "one-graph", "eager"])
def test_census_log_shows_every_generation_of_a_chunk(run, side, kind):
    """one evolve(4) -- a replayed 4-generation chunk (two graphs: generations 0..2 counted by the next
    run launch's extra workgroups; one graph: on the side stream) or four eager generations (side
    stream) -- logs the census and the newborn count of each of its generations; the last is the
    join's.  Expected rows: a twin stepped with four evolve(1) calls"""
    for n in (130, 3000):
        o, _ = population(kind, n, device="cuda", execution=_exec("stream", run == "two-graph", side, "batch"))
        o.census_log = True
        skip = 0
        if run != "eager":
            assert o.capture(warmup=1)
            skip = 1
            ch = next(c for c in o._chunks if c[2] == 4 and c[1] == o._p)  # the chunk evolve(4) replays
            assert (ch[3] is not None) == (run == "two-graph")
        assert o._ord_census_side == side
        o.evolve(4)
        want, t = _twin_rows(kind, n, skip, 4)
        got = o.census_history()
        assert got.shape == (4, 6)
        assert torch.equal(got, want), (got.tolist(), want.tolist())
        assert all(int(r[:5].sum()) == n for r in got)
        if kind == "seeded":
            assert all(int((r[:5] > 0).sum()) == 5 for r in want)
        else:
            assert int(want[:, 5].min()) > 0  # every generation of the HOT soup respawned somebody
        assert o.last_census() == t.count() and int(o.counts[5]) == int(want[3, 5])
        assert torch.equal(o.uid, t.uid) and int(o.next_uid[0]) == int(t.next_uid[0])
        assert o.ordered_levels()["error"] == 0
        o.release_graphs()


def test_census_log_of_the_one_workgroup_finish_and_shorter_launches():
    """finish_par=False (k_gen_finish_batch walks the generations in one workgroup) writes the same
    rows; a shorter finish launch (a 2-generation chunk, a single-generation graph) logs its own
    generations from row 0; the log is switched on or off before capture() only"""
    n = 130
    o, _ = population("seeded", n, device="cuda", execution=_exec("stream", True, True, "batch", finish_par=False))
    o.census_log = True
    assert o.capture(warmup=1)
    want, _ = _twin_rows("seeded", n, 1, 7)
    o.evolve(4)
    assert torch.equal(o.census_history(), want[0:4])
    o.evolve(2)
    assert torch.equal(o.census_history(), want[4:6])
    o.evolve(1)
    assert torch.equal(o.census_history(), want[6:7])
    with pytest.raises(ValueError, match="before capture"):  # (the graphs write the log's buffer)
        o.census_log = False
    o.release_graphs()
    o.census_log = False
    assert o._census_log is None
    late, _ = population("seeded", n, device="cuda", execution=_exec("stream", True, True, "batch"))
    assert late.capture(warmup=1)
    with pytest.raises(ValueError, match="before capture"):
        late.census_log = True
    late.release_graphs()
