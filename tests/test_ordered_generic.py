"""Reference-order soups of runtime shapes (csrc/srnn_generic.hip GOrd / g_soup_ordered): the
continuation-scheduled generation of csrc/srnn_ordered.h with the runtime-shape engine's turn, for
every shape without a lane template -- WW(3,3), Agg(4,3,2), RNN(3,2), FFT(3,2,2) here.  Host path:
bitwise the serial loop (SequentialSoupEngine), census and counts in the close, routing, memory
accounting, recording."""
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.config import ExecConfig
from self_replicating_neural_networks_amd.models import network as N
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.seq_soup import SequentialSoupEngine
from self_replicating_neural_networks_amd.soup import Soup
from self_replicating_neural_networks_amd.soup_engine import SoupEngine, _finish_batch, engine_bytes

SPECS = [ArchSpec.weightwise(3, 3), ArchSpec.aggregating(4, 3, 2), ArchSpec.recurrent(3, 2), ArchSpec.fft(3, 2, 2)]
IDS = ["ww33", "agg432", "rnn32", "fft322"]
HOT = dict(attacking_rate=0.3, learn_from_rate=0.3, train=2, learn_from_severity=2, remove_divergent=True,
           remove_zero=True, epsilon=1e-4)
N_SOUP, SEED, GENS = 300, 5, 4


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _same(ordered: SoupEngine, seq: SequentialSoupEngine, P: int):
    assert torch.equal(_bits(ordered.local_rows()[:, :P]), _bits(seq.W[:, :P]))
    assert torch.equal(ordered.uid.cpu(), seq.uid.cpu())
    assert int(ordered.next_uid[0]) == int(seq.next_uid[0])
    assert torch.equal(ordered.action.cpu(), seq.action.cpu())
    assert torch.equal(ordered.counterpart.cpu(), seq.counterpart.cpu())
    assert torch.equal(ordered.respawn.cpu(), seq.respawn.cpu())
    assert torch.equal(_bits(ordered.loss), _bits(seq.loss))


_SERIAL = {}


def _serial(spec):
    """the serial loop's state after each generation, computed once per shape"""
    if spec not in _SERIAL:
        s = SequentialSoupEngine(spec, N_SOUP, HOT, seed=SEED)
        snaps = []
        for _ in range(GENS + 1):
            snaps.append(dict(W=s.W.clone(), uid=s.uid.clone(), next_uid=s.next_uid.clone(), action=s.action.clone(),
                              counterpart=s.counterpart.clone(), respawn=s.respawn.clone(), loss=s.loss.clone()))
            s.evolve(1)
        _SERIAL[spec] = snaps
    return _SERIAL[spec]


class _Snap:
    def __init__(self, d):
        self.__dict__.update(d)


def test_runtime_shapes_are_routed_to_the_ordered_generation():
    for spec in SPECS + [ArchSpec.weightwise(10, 3), ArchSpec.weightwise(16, 2), ArchSpec.aggregating(4, 4, 3),
                         ArchSpec.recurrent(8, 2)]:
        for dev in (False, True):
            assert _lib.supports(spec, _lib.OP_SOUP_ORDERED, dev), (spec, dev)
            assert _lib.supports(spec, _lib.OP_ORD_PLAN, dev), (spec, dev)
            assert not _lib.supports(spec, _lib.OP_ORD_CENSUS, dev)  # the census stays in the close
    big = ArchSpec.aggregating(4, 10, 3)  # unchanged: device only
    assert _lib.supports(big, _lib.OP_SOUP_ORDERED, True) and not _lib.supports(big, _lib.OP_SOUP_ORDERED, False)
    # no device serial loop for runtime shapes
    assert not _lib.supports(ArchSpec.weightwise(3, 3), _lib.OP_SOUP_SEQ, True)
    # a Weightwise coordinate table past the run launch's static LDS is refused (device)
    wide = ArchSpec.weightwise(32, 3)
    assert wide.P > 1024
    assert not _lib.supports(wide, _lib.OP_SOUP_ORDERED, True) and _lib.supports(wide, _lib.OP_SOUP_ORDERED, False)
    # the run launch: one lane per turn plus the critical-list waves
    assert _lib.ord_run_lanes(100000) >= 100000 and _lib.ord_run_lanes(100000) % 64 == 0
    assert _lib.generic_ord_scratch_bytes(SPECS[0], 1500) > _lib.generic_ord_scratch_bytes(SPECS[0], 100)


@pytest.mark.parametrize("spec", SPECS, ids=IDS)
@pytest.mark.parametrize("levels", [1, 4])
@pytest.mark.parametrize("pipe", ["off", "stream", "kernel"])
def test_host_ordered_generation_of_a_runtime_shape_is_the_serial_loop(spec, levels, pipe):
    """host OP_SOUP_ORDERED of a runtime shape == OP_SOUP_SEQ bitwise after every generation (rows,
    uid, next_uid, action, counterpart, respawn, loss bits); census == count() and counts[5] == the
    respawn flags, each generation"""
    o = SoupEngine(spec, N_SOUP, HOT, device="cpu", seed=SEED, order="sequential",
                   execution=ExecConfig(order_levels=levels, ord_pipeline=pipe))
    assert o._ord_mode == pipe and o._ord_generic
    o.stats = True
    snaps = _serial(spec)
    _same(o, _Snap(snaps[0]), spec.P)
    deep = 0
    for g in range(1, GENS + 1):
        o.evolve(1)
        _same(o, _Snap(snaps[g]), spec.P)
        lv = o.ordered_levels()
        deep = max(deep, lv["max_level"])
        assert lv["error"] == 0
        assert o.last_census() == o.count()
        assert int(o.counts[5]) == int((o.respawn != 0).sum())
    assert deep >= 2  # real dependency chains ran


def _ww33_trainer():
    return N.TrainingNeuralNetworkDecorator(N.WeightwiseNeuralNetwork(3, 3)).with_params(epsilon=1e-4)


def test_soup_auto_mode_keeps_a_runtime_shape_on_the_scheduled_generation():
    s = Soup(500, _ww33_trainer)
    assert s.mode == "ordered"
    s.with_params(train=1, remove_divergent=True, remove_zero=True)
    s.seed()
    assert isinstance(s.engine, SoupEngine) and s.engine.order == "sequential" and s.mode == "ordered"
    s.evolve(1)
    assert sum(s.count().values()) == 500


def test_big_aggregating_nets_still_have_no_host_form():
    with pytest.raises(NotImplementedError, match="SequentialSoupEngine"):
        SoupEngine(ArchSpec.aggregating(4, 10, 3), 10, HOT, device="cpu", order="sequential")


def _held_bytes(e: SoupEngine) -> int:
    seen, total = set(), 0
    for t in e._state() + [e._scratch]:
        if t is None or t.data_ptr() in seen:
            continue
        seen.add(t.data_ptr())
        total += t.numel() * t.element_size()
    return total


@pytest.mark.parametrize("n", [1000, 64])
def test_engine_bytes_counts_the_run_scratch_of_a_runtime_shape(n):
    spec = ArchSpec.weightwise(3, 3)
    e = SoupEngine(spec, n, dict(train=1), device="cpu", order="sequential")
    est = engine_bytes(spec, n, order="sequential", epochs=2)
    held = _held_bytes(e)
    # GPU-only buffers a host engine does not hold: the batched-finish ring and the scratch lanes
    assert e._bs_ring is None and e._scratch is None and e._perm_table() is None
    nb = max(-(-n // 64), 1)
    held += _finish_batch(nb, e._chunk_sizes()) * (nb * 8 + 2) * 4
    scratch = max(_lib.generic_scratch_bytes(spec, n), _lib.generic_ord_scratch_bytes(spec, n))
    assert scratch >= _lib.ord_run_lanes(n) * 4 * 4 * spec.PP  # at least four row vectors per run lane
    held += scratch
    assert est >= held * 0.99 and est <= held * 1.05 + 512, (est, held)
    assert est >= engine_bytes(ArchSpec.weightwise(2, 2), n, order="sequential", epochs=0) + scratch


def test_ordered_soup_of_a_runtime_shape_records_reference_states():
    s = Soup(150, _ww33_trainer, mode="ordered", seed=4, record=True).with_params(
        attacking_rate=0.3, learn_from_rate=0.2, train=1, remove_divergent=True, remove_zero=True)
    s.seed()
    assert isinstance(s.engine, SoupEngine) and s.mode == "ordered"
    s.evolve(3)
    n_states = sum(len(p.get_states()) for p in s.historical_particles.values())
    assert n_states >= 150 * 3
    acts = {st.get("action") for p in s.historical_particles.values() for st in p.get_states()}
    assert {"init", "train_self"} <= acts
