"""Reference-order soups of runtime shapes on the device (csrc/srnn_generic.hip: GOrd, GOrdPol in
k_ord_run and k_ord_close):

A. the template shapes forced onto the runtime-shape path == the template engine on the same device,
   bitwise, eager and graph-captured (the template side is proven bitwise the serial loop);
B. shapes without a template == the host serial loop (SequentialSoupEngine) from the same rows;
C. hipGraph chunks (one- and two-graph form) == an eager twin; serial == batched finish;
D. a scratch buffer shorter than the run launch needs is refused before anything is launched."""
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


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def canon(t):
    """Bit pattern of a tensor with every NaN mapped to one value (NaN payloads are not a contract)."""
    t = torch.nan_to_num(t.float().cpu(), 7.0, 9.0, -9.0).contiguous()
    return t.view(torch.int32)


class _forced:
    """the process-global SRNN_KNOB_FORCE_GENERIC around one engine's calls"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib.set_force_generic(self.on)

    def __exit__(self, *exc):
        _lib.set_force_generic(False)


def _same_engines(a: SoupEngine, b: SoupEngine, P: int):
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.local_rows()[:, :P]), _bits(b.local_rows()[:, :P]))
    assert torch.equal(a.uid, b.uid) and int(a.next_uid[0]) == int(b.next_uid[0])
    assert torch.equal(a.action, b.action) and torch.equal(a.counterpart, b.counterpart)
    assert torch.equal(a.respawn, b.respawn)
    assert torch.equal(_bits(a.loss), _bits(b.loss))
    assert a.last_census() == b.last_census()
    assert a.ordered_levels()["error"] == 0 and b.ordered_levels()["error"] == 0


# ---------------------------------------------------------------- A. same-device oracle
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("spec", [ArchSpec.weightwise(2, 2), ArchSpec.aggregating(4, 2, 2), ArchSpec.recurrent(2, 2)],
                         ids=["ww22", "agg422", "rnn22"])
def test_forced_runtime_path_equals_the_template_generation(spec, graphs):
    n, seed = 1500, 7  # (not a multiple of 64)
    ex = ExecConfig(graph_chunks=(4, 2))
    try:
        with _forced(True):
            g = SoupEngine(spec, n, HOT, device="cuda", seed=seed, order="sequential", execution=ex)
            assert g._ord_generic and g._scratch is not None
            assert g._scratch.numel() >= _lib.generic_ord_scratch_bytes(spec, n)
        t = SoupEngine(spec, n, HOT, device="cuda", seed=seed, order="sequential", execution=ex,
                       weights=g.local_rows()[:, :spec.P].cpu())
        assert not t._ord_generic
        g.stats = t.stats = True
        if graphs:
            with _forced(True):
                assert g.capture(warmup=1)
            assert t.capture(warmup=1)
            _same_engines(g, t, spec.P)
        for k in (1, 2, 4):
            with _forced(True):
                g.evolve(k)
                torch.cuda.synchronize()
            t.evolve(k)
            _same_engines(g, t, spec.P)
        assert sum(g.last_census().values()) == n
        g.release_graphs()
        t.release_graphs()
    finally:
        _lib.set_force_generic(False)


# ---------------------------------------------------------------- B. runtime shapes vs the host serial loop
def _against_host_loop(spec, params, n=1200, seed=11, gens=3):
    assert _lib.is_generic(spec, _lib.OP_SOUP_ORDERED)
    o = SoupEngine(spec, n, params, device="cuda", seed=seed, order="sequential")
    assert o._ord_generic
    o.stats = True
    s = SequentialSoupEngine(spec, n, params, seed=seed, weights=o.local_rows()[:, :spec.P].float().cpu())
    deep = 0
    for g in range(gens):
        o.evolve(1)
        s.evolve(1)
        torch.cuda.synchronize()
        assert torch.equal(o.action.cpu(), s.action.cpu()), g
        assert torch.equal(o.counterpart.cpu(), s.counterpart.cpu()), g
        assert torch.equal(o.respawn.cpu(), s.respawn.cpu()), g
        assert torch.equal(o.uid.cpu(), s.uid.cpu()), g
        bad = int((canon(o.local_rows()[:, :spec.P]) != canon(s.W[:, :spec.P])).any(dim=1).sum())
        print(f"{spec} generation {g}: rows that differ from the host loop {bad}/{n}")
        assert bad == 0, g
        assert torch.equal(_bits(o.loss), _bits(s.loss)), g
        lv = o.ordered_levels()
        assert lv["error"] == 0
        deep = max(deep, lv["max_level"])
        census = o.last_census()
        assert census == o.count() and sum(census.values()) == n, g
        assert int(o.counts[5]) == int((o.respawn != 0).sum()), g
    assert deep >= 2
    assert int(o.next_uid[0]) == int(s.next_uid[0])


@pytest.mark.parametrize("spec", [ArchSpec.weightwise(3, 3), ArchSpec.aggregating(4, 4, 3), ArchSpec.fft(3, 2, 2)],
                         ids=["ww33", "agg443", "fft322"])
def test_device_ordered_runtime_shape_is_the_host_serial_loop(spec):
    """rows (NaNs canonicalised), uid, action, counterpart, respawn and loss bits == the host serial loop.

    The FFT case needs the cosine factors of the FFT nets to be the same bits on both sides (cos_hd,
    csrc/srnn_core.h): with libm's cosf -- glibc's on the host, the device library's on the GPU -- an FFT
    attack differed between host and device in the last bit (278/1200 rows after one generation)."""
    _against_host_loop(spec, HOT)


def test_device_ordered_recurrent_runtime_shape_is_the_host_serial_loop():
    """RNN(3,2) without respawn: a newborn's orthogonal init goes through the device's libm and is not
    bitwise the host's (case A covers the respawn of the recurrent kind on one device)"""
    _against_host_loop(ArchSpec.recurrent(3, 2), dict(HOT, remove_divergent=False, remove_zero=False))


# ---------------------------------------------------------------- C. graphs equal eager
@pytest.mark.parametrize("sync", [True, False], ids=["graph-sync-on", "graph-sync-off"])
@pytest.mark.parametrize("spec", [ArchSpec.weightwise(3, 3), ArchSpec.recurrent(3, 2)], ids=["ww33", "rnn32"])
def test_device_ordered_runtime_shape_graphs_equal_eager(spec, sync):
    """chunks of 2 and 4 and single-generation graphs == an eager twin, with ord_graph_sync on and off.
    A runtime shape keeps the one-graph form of a chunk either way: the counter waits of a two-graph
    chunk give up after ~2 s, which one generation of a wide runtime shape at 100k particles passes
    (profiles/ordered_runtime_shapes.md)."""
    n, seed = 1500, 3
    ex = ExecConfig(ord_pipeline="stream", ord_graph_sync=sync, graph_chunks=(4, 2))
    a = SoupEngine(spec, n, HOT, device="cuda", seed=seed, order="sequential", execution=ex)
    b = SoupEngine(spec, n, HOT, device="cuda", seed=seed, order="sequential", execution=ex)
    a.stats = b.stats = True
    assert b.capture(warmup=1)
    assert sorted(c[2] for c in b._chunks if c[1] == b._p) == [2, 4]
    assert not any(c[3] is not None for c in b._chunks) and not b._ord_decouple
    a.evolve(1)
    _same_engines(a, b, spec.P)
    for k in (2, 4, 1, 2):  # chunks of 2 and 4, a single-generation graph between them
        a.evolve(k)
        b.evolve(k)
        _same_engines(a, b, spec.P)
    assert b.last_census() == b.count() and sum(b.last_census().values()) == n
    assert int(a.counts[5]) == int(b.counts[5]) == int((b.respawn != 0).sum())
    b.release_graphs()


def test_device_ordered_runtime_shape_serial_and_batched_finish_agree():
    spec, n = ArchSpec.weightwise(3, 3), 1500
    es = [SoupEngine(spec, n, HOT, device="cuda", seed=4, order="sequential", execution=ExecConfig(finish_mode=fm))
          for fm in ("serial", "batch")]
    assert [e.finish_mode for e in es] == ["serial", "batch"]
    for e in es:
        e.stats = True
        e.evolve(3)
    _same_engines(es[0], es[1], spec.P)
    assert torch.equal(es[0].counts, es[1].counts)
    assert es[0].last_census() == es[0].count()


# ---------------------------------------------------------------- D. short scratch
def test_short_scratch_is_refused_before_any_launch():
    spec, n = ArchSpec.weightwise(3, 3), 1500
    o = SoupEngine(spec, n, HOT, device="cuda", seed=1, order="sequential", execution=ExecConfig(ord_pipeline="off"))
    need = _lib.generic_ord_scratch_bytes(spec, n)
    assert need > _lib.generic_scratch_bytes(spec, n)  # more lanes than the other operators' launches
    rows0 = o.local_rows().clone()
    _, ca, _ = o._gen_args()
    ca.scratch_bytes = need - 1
    with pytest.raises(_lib.NativeLibraryError, match="scratch"):
        _lib.run(_lib.OP_SOUP_ORDERED, spec, ca, o.cfg)
    ca.scratch_bytes = o._scratch.numel()
    torch.cuda.synchronize()
    assert torch.equal(o.local_rows(), rows0) and o.ordered_error() == 0
    o.evolve(1)  # the same argument block with its full scratch runs
    assert o.ordered_levels()["error"] == 0
