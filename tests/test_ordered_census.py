"""The census of a reference-order soup (SoupEngine(order="sequential"), stats = True) against
oracles that share nothing with it.  ``last_census()`` -- counts[0:5], reduced by the finish from the
packed class counts the close (or a deferred census) left in the block stats -- must equal

  * ``count()``: the stand-alone classify kernel on the final rows, no block stats involved,
  * the serial loop's ``count()`` (SequentialSoupEngine stepped alongside, rows bitwise equal),
  * on the host, the per-row numpy reference ``oracle.core.classify`` histogrammed,

and counts[5] (the respawn ballots, word 0 of the block stats) must equal the respawn flags set and
the advance of next_uid.  The HOT soup of tests/test_ordered_soup.py only ever shows fix_zero and
other (a few divergent for the RNN), so a second, seeded Weightwise(2, 2) population keeps all five
classes non-empty: zero rows, NaN rows, the identity fixpoint, small perturbations of it, and the
negated identity f(x) = -x, an exact second-order fixpoint (tests/classify_rows.py) -- the high half of
block-stat word 2.  Every fourth row starts as one; enough of them stay unattacked for fix_sec to
be non-empty at each of the 17 first generations at every size of SIZES.  The device counterpart
is tests/test_ordered_census_gpu.py."""
import numpy as np
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.config import ExecConfig
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.oracle import core as oc
from self_replicating_neural_networks_amd.seq_soup import SequentialSoupEngine
from self_replicating_neural_networks_amd.setups.experiments import identity_fixpoint_weights
from self_replicating_neural_networks_amd.soup_engine import SoupEngine
from classify_rows import path_row
from test_ordered_soup import HOT, IDS, SPECS, _same

WW = ArchSpec.weightwise(2, 2)
SEEDED = dict(attacking_rate=0.05, learn_from_rate=0.05, train=0, remove_divergent=False, remove_zero=False,
              epsilon=1e-4)
# one partial 64-row block, exactly one, two + a 2-row tail, 46 + one of 56 rows (real dependency chains)
SIZES = [37, 64, 130, 3000]
SEED = 5


def seeded_rows(n: int) -> torch.Tensor:
    """The seeded Weightwise(2, 2) population: the keyed initial rows with negated identities (fix_sec),
    zero rows, NaN rows, identity fixpoints and fixpoints perturbed by 3e-5 * randn written over them
    (later writes win)."""
    W = torch.zeros((n, WW.PP), dtype=torch.float32)
    K.init_rows(WW, W, torch.arange(n, dtype=torch.int64), SEED)
    W = W[:, :WW.P].clone()
    fix = torch.from_numpy(identity_fixpoint_weights())
    W[2::4] = torch.from_numpy(path_row(WW, -1.0, 1.0, 0))
    W[0::7] = 0.0
    W[1::11, 0] = float("nan")
    W[3::5] = fix
    g = torch.Generator().manual_seed(1234)
    noise = 3e-5 * torch.randn((n, WW.P), generator=g)
    W[4::10] = fix + noise[4::10]
    return W


def population(kind, n, device="cpu", **kw):
    """(ordered engine with stats, serial engine from the same rows, params); kind: a spec of SPECS
    (the HOT soup from its keyed initial rows) or "seeded"."""
    if isinstance(kind, str):
        spec, params, rows = WW, SEEDED, seeded_rows(n)
        o = SoupEngine(spec, n, params, device=device, seed=SEED, order="sequential", weights=rows, **kw)
    else:
        spec, params = kind, HOT
        o = SoupEngine(spec, n, params, device=device, seed=SEED, order="sequential", **kw)
        # (the same starting rows: the device init contracts a*b+c, the host's does not)
        rows = o.local_rows()[:, :spec.P].cpu()
    o.stats = True
    s = SequentialSoupEngine(spec, n, params, seed=SEED, device=device, weights=rows)
    return o, s


def check_census(o, s, uid_before=None, with_sec=True, min_classes=1, numpy_rows=False):
    """Every identity of the module docstring after an evolve call; ``uid_before``: next_uid before
    a one-generation call; ``min_classes``: non-empty classes the oracle's census must show (a
    population collapsed to one class cannot pass a five-class test)."""
    n = o.n
    got = o.last_census()
    want = s.count(with_sec=with_sec)
    assert sum(v > 0 for v in want.values()) >= min_classes, want
    assert got == want, "census of the generation != census of the serial loop's rows"
    assert got == o.count(with_sec=with_sec), "census of the generation != classify kernel on its final rows"
    assert sum(got.values()) == n
    born = int(o.counts[5])
    assert born == int((o.respawn != 0).sum()) == int((s.respawn != 0).sum())
    if uid_before is not None:
        assert born == int(o.next_uid[0]) - uid_before
    if numpy_rows:  # (host rows only: the device contracts a*b+c, rows on the epsilon boundary may differ)
        rows = o.local_rows()[:, :o.spec.P].float().cpu().numpy()
        assert got == oc.counts_of(oc.classify(o.spec, rows, o.eps, with_sec=with_sec))
    return got


KINDS = list(zip(SPECS, IDS)) + [("seeded", "seeded")]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", [k for k, _ in KINDS], ids=[i for _, i in KINDS])
@pytest.mark.parametrize("pipe", ["kernel", "stream", "off"])
def test_host_ordered_census_equals_independent_oracles(pipe, kind, n):
    o, s = population(kind, n, execution=ExecConfig(ord_pipeline=pipe))
    assert o._ord_mode == pipe
    seeded = kind == "seeded"
    deep = 0
    for _ in range(4):
        uid0 = int(o.next_uid[0])
        o.evolve(1)
        s.evolve(1)
        _same(o, s, o.spec.P)
        check_census(o, s, uid_before=uid0, min_classes=5 if seeded else 1, numpy_rows=True)
        deep = max(deep, o.ordered_levels()["max_level"])
    if n == 3000 and not seeded:
        assert deep >= 2  # real dependency chains
        assert int(o.next_uid[0]) > n  # the HOT soup respawned: the ballots counted something
    assert o.ordered_levels()["error"] == 0


def test_host_ordered_census_without_second_order_fixpoints():
    """stats_with_sec = False against count(with_sec=False), and a multi-generation evolve (counts
    describe its last generation)"""
    o, s = population("seeded", 130)
    o.stats_with_sec = False
    for k in (1, 3):
        o.evolve(k)
        s.evolve(k)
        got = check_census(o, s, with_sec=False, min_classes=4, numpy_rows=True)
        # the second-order fixpoints are there and are counted as other
        sec = s.count(with_sec=True)
        assert got["fix_sec"] == 0 < sec["fix_sec"] and got["other"] == sec["other"] + sec["fix_sec"]


def test_deferred_census_without_batched_finish_is_rejected():
    """SRNN_F_ORD_CENSUS_LATER leaves the class counts to a later launch; without SRNN_F_GEN_COUNTS
    (the batched finish) the finish follows the close at once and would report zeros: the library
    refuses the combination instead (-5), and the refused call changed nothing"""
    o, s = population("seeded", 130)
    o.evolve(1)
    s.evolve(1)
    _, ca, _ = o._gen_args()
    assert not ca.flags & (_lib.FLAG_ORD_CENSUS_LATER | _lib.FLAG_GEN_COUNTS)
    bad = _lib.SrnnArgs.from_buffer_copy(ca)
    bad.flags = ca.flags | _lib.FLAG_ORD_CENSUS_LATER
    with pytest.raises(_lib.NativeLibraryError, match=r"\(-5\).*SRNN_F_ORD_CENSUS_LATER needs the batched finish"):
        _lib.run(_lib.OP_SOUP_ORDERED, o.spec, bad, o.cfg)
    bad.flags |= _lib.FLAG_GEN_COUNTS  # (the pair the engine sets passes the check)
    assert np.array_equal(o.local_rows().numpy().view(np.int32), s.W.numpy().view(np.int32))
    o.evolve(1)
    s.evolve(1)
    _same(o, s, o.spec.P)
    check_census(o, s, min_classes=5)


def test_census_log_needs_the_batched_finish():
    """the per-generation census log rides on the batched finish (a GPU engine's): the host engine,
    whose generation call finishes inline, refuses it; off by default"""
    o, _ = population("seeded", 64)
    assert o.census_log is False
    with pytest.raises(ValueError, match="finish_mode='batch'"):
        o.census_log = True
    with pytest.raises(RuntimeError, match="census_log is off"):
        o.census_history()
