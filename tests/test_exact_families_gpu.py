"""Every device kernel route of the Aggregating and Recurrent families against the exact float32
oracle (oracle/exact.py) at ZERO tolerance -- directly, not through another kernel:

=========================  ==========================================================  =====
route                      shapes                                                      rows
=========================  ==========================================================  =====
templated lane (k_op)      Agg(4,2,2) mean / max / max_ref / shuffle_random,           131
                           Agg(2,2,2), RNN(2,2), RNN(1,1)
runtime-shape lane         Agg(4,2,2) (+ max_ref, shuffle_random) and RNN(2,2) forced  131
                           generic; Agg(4,4,3), RNN(3,2)
big-net row kernels        Agg(4,10,3) (+ shuffle_random), Agg(4,8,2) max, Agg(4,16,2) 131, 1
Recurrent wave, specialised  RNN(8,2)                                                  37
Recurrent wave, runtime    RNN(12,3); RNN(8,2) with the specialisations off            37
=========================  ==========================================================  =====

131 rows are two waves and a 3-lane tail; one row is a partly filled LDS staging pass of the row
kernels.  Per route (tests/exact_ops.py): the device init (Aggregating) == the oracle's; a
self-application; an attack through idx_f / idx_t / idx_o; run_fixpoint(3, early_exit=False) ==
three exact applies with nsteps == 3 (the chunk-state shortcut of k_big_fix*); three self-train
epochs with their loss; two learn_from epochs through a gather.  Recurrent rows are the host
init scaled by 0.5: every compared row is finite (asserted), so the second and third BPTT epoch
are compared on numbers, not on inf / NaN patterns.  Each case asserts the route it means to take.

Reference-order generations (SoupEngine(order="sequential")) of Agg(4,4,3) (lane turn),
Agg(4,10,3) (BigOrd) and RNN(8,2) (k_gord_run_rnn, respawn off) == ``seq_generation``,
generation by generation from the device's own rows."""
import numpy as np
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.oracle import core as C
from self_replicating_neural_networks_amd.oracle import exact as X
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.soup_engine import SoupEngine

import exact_ops as E

pytestmark = pytest.mark.gpu

AGG = ArchSpec.aggregating
RNN = ArchSpec.recurrent
OPS = (_lib.OP_APPLY, _lib.OP_RUN_FIXPOINT, _lib.OP_TRAIN, _lib.OP_LEARN)
sid = lambda s: f"{s.kind[:3]}{s.aggregates or ''}-{s.width}-{s.depth}-{s.aggregator}-{s.shuffler}"
LANE = [AGG(4, 2, 2), AGG(4, 2, 2, "max"), AGG(4, 2, 2, "max_ref"), AGG(4, 2, 2, shuffler="random"), AGG(2, 2, 2),
        RNN(2, 2), RNN(1, 1)]


@pytest.mark.parametrize("spec", LANE, ids=sid)
def test_templated_lane_kernels(cuda, spec):
    assert not any(_lib.is_generic(spec, op) for op in OPS) and not K.is_wave_per_particle(spec)
    assert _lib.train_form(spec) == "lane"
    E.check_ops(spec, 131, cuda)


@pytest.mark.parametrize("spec", [AGG(4, 2, 2), AGG(4, 2, 2, "max_ref"), AGG(4, 2, 2, shuffler="random"), RNN(2, 2)],
                         ids=sid)
def test_runtime_shape_lane_engine_forced(cuda, spec):
    _lib.set_force_generic(True)
    try:
        assert all(_lib.is_generic(spec, op) for op in OPS) and _lib.train_form(spec) == "lane"
        E.check_ops(spec, 131, cuda)
    finally:
        _lib.set_force_generic(False)


@pytest.mark.parametrize("spec", [AGG(4, 4, 3), RNN(3, 2)], ids=sid)
def test_runtime_shape_lane_engine(cuda, spec):
    assert all(_lib.is_generic(spec, op) for op in OPS) and _lib.train_form(spec) == "lane"
    E.check_ops(spec, 131, cuda)


@pytest.mark.parametrize("n", [131, 1])
@pytest.mark.parametrize("spec", [AGG(4, 10, 3), AGG(4, 10, 3, shuffler="random"), AGG(4, 8, 2, "max"), AGG(4, 16, 2)],
                         ids=sid)
def test_big_net_row_kernels(cuda, spec, n):
    assert not any(_lib.is_generic(spec, op) for op in (_lib.OP_APPLY, _lib.OP_TRAIN, _lib.OP_LEARN))
    assert _lib.train_form(spec) == "wave"
    assert _lib.get_knob("big_wave") != 1  # the lane-per-particle row kernels, not the wave-per-particle ones
    W = torch.zeros(n, spec.PP, device=cuda)
    # run_fixpoint: the chunk-state kernels for the unshuffled nets, the runtime-shape engine for shuffle_random
    assert K.needs_chunk_state_temp(spec, W) == (spec.shuffler == "none")
    assert K.is_wave_per_particle(spec, W) == (spec.shuffler == "none")
    E.check_ops(spec, n, cuda)


def test_recurrent_wave_specialised(cuda):
    spec = RNN(8, 2)
    assert _lib.get_knob("rnn_wave") != 0 and _lib.get_knob("rnn_spec") != 0
    assert _lib.train_form(spec) == "wave" and all(_lib.is_generic(spec, op) for op in OPS)
    E.check_ops(spec, 37, cuda)


@pytest.mark.parametrize("spec", [RNN(12, 3), RNN(8, 2)], ids=sid)
def test_recurrent_wave_runtime_shape(cuda, spec):
    _lib.set_rnn_spec(False)
    try:
        assert _lib.get_knob("rnn_wave") != 0 and _lib.get_knob("rnn_spec") == 0
        assert _lib.train_form(spec) == "wave"
        E.check_ops(spec, 37, cuda)
    finally:
        _lib.set_rnn_spec(True)


def test_recurrent_lane_path_of_a_wide_net(cuda):
    """the lane twin the wave kernels are compared with elsewhere (set_rnn_wave(False)) == the oracle too"""
    spec = RNN(8, 2)
    _lib.set_rnn_wave(False)
    try:
        assert _lib.get_knob("rnn_wave") == 0 and _lib.train_form(spec) == "lane"
        E.check_ops(spec, 37, cuda)
    finally:
        _lib.set_rnn_wave(True)


# ------------------------------------------------------------------ reference-order generations
SOUP = dict(attacking_rate=0.3, learn_from_rate=0.3, train=2, learn_from_severity=2, epsilon=1e-4)
RESPAWN = dict(SOUP, remove_divergent=True, remove_zero=True)
NO_RESPAWN = dict(SOUP, remove_divergent=False, remove_zero=False)


@pytest.mark.parametrize("spec,params,generic,form", [(AGG(4, 4, 3), RESPAWN, True, "lane"),
                                                      (AGG(4, 10, 3), RESPAWN, False, None),
                                                      (RNN(8, 2), NO_RESPAWN, True, "wave")],
                         ids=["agg443-lane", "agg4103-bigord", "rnn82-wave"])
def test_device_reference_order_generations(cuda, spec, params, generic, form):
    """two device reference-order generations == ``seq_generation``: rows, actions, counterparts,
    respawns and loss bits, each generation from the device's own rows"""
    n, seed = 96, 5
    rows0 = None
    if spec.kind == "recurrent":  # half the init scale: every row stays finite
        rows0 = SoupEngine(spec, n, params, device="cuda", seed=seed,
                           order="sequential").local_rows()[:, :spec.P].float().cpu() * 0.5
    o = SoupEngine(spec, n, params, device="cuda", seed=seed, order="sequential", weights=rows0)
    assert o._ord_generic == generic and (form is None or o.ordered_run_form() == form)
    W = o.local_rows()[:, :spec.P].cpu().numpy().copy()
    att, te = C.soup_decisions(seed, 1, n, params["attacking_rate"], params["learn_from_rate"])
    assert (att >= 0).sum() > 10 and (te >= 0).sum() > 10  # attacks and learn_from turns occur
    if spec.kind != "recurrent":
        E.assert_bits(W, X.init(spec, np.arange(n), seed), "init")
    for g in range(1, 3):
        W, act, cp, loss, rs = X.seq_generation(spec, W, g, seed, params)
        o.evolve(1)
        torch.cuda.synchronize()
        assert o.ordered_levels()["error"] == 0
        got = o.local_rows()[:, :spec.P].cpu().numpy()
        assert E.finite_share(W) >= 0.9
        E.assert_bits(got, W, f"{spec} generation {g}")
        assert np.array_equal(o.action.cpu().numpy(), act) and np.array_equal(o.counterpart.cpu().numpy(), cp)
        assert np.array_equal(o.respawn.cpu().numpy(), rs)
        E.assert_bits(o.loss, loss, f"{spec} generation {g} loss")
        assert (act == 3).all()  # train=2: every turn ends self-training
        W = got.copy()
