"""Mixed runs on the device: the fused OP_RUN_MIXED launch against the op sequence on device tables
and against the host's fused run, bit for bit; the shapes whose training has a wave kernel, where
``run_mixed`` keeps the op sequence; ``MixedFixpointExperiment.run_population`` on a device
population."""
import pytest
import torch

from self_replicating_neural_networks_amd.experiment import MixedFixpointExperiment
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.population import Population

from classify_rows import sid
from test_mixed_run import (AGG, CTR, EPS, RNN, SEED, STEPS, WW, assert_not_degenerate, assert_same, bits,
                            population, run_both)

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(WW(2, 2), torch.float32), (WW(2, 2), torch.bfloat16), (AGG(4, 2, 2, shuffler="random"), torch.float32),
         (RNN(2, 2), torch.float32), (WW(3, 3), torch.float32), (AGG(4, 4, 3), torch.float32)]


def case_id(c):
    return sid(c[0]) + ("-bf16" if c[1] == torch.bfloat16 else "")


@pytest.mark.parametrize("check_first", [True, False], ids=["checked", "step0-free"])
@pytest.mark.parametrize("trains", [0, 3])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fused_equals_op_sequence_on_device(case, trains, check_first):
    spec, dtype = case
    record = spec in (WW(2, 2), WW(3, 3)) and dtype == torch.float32
    for n in (None, 1, 65):
        W, uid = population(spec, dtype, n=n, device=DEV)
        f, o = run_both(spec, W, uid, trains, check_first, record, fused=K.run_mixed_fused)
        if n is None:
            assert_not_degenerate(o[1][1], check_first)
        assert_same(f, o, record)


@pytest.mark.parametrize("spec", [WW(2, 2), WW(3, 3)], ids=sid)
def test_device_equals_host(spec):
    """the host is built with the device's contraction: the same fused run, the same bits"""
    for trains, check_first in ((0, True), (3, True), (3, False)):
        Wh, uh = population(spec)
        Wd, ud = population(spec, device=DEV)
        args = dict(check_first=check_first, record=True, seed=SEED, ctr=CTR)
        rh = K.run_mixed_fused(spec, Wh, trains, STEPS, EPS, uid=uh, **args)
        rd = K.run_mixed_fused(spec, Wd, trains, STEPS, EPS, uid=ud, **args)
        assert_same((Wd, rd), (Wh, rh), record=True)


@pytest.mark.parametrize("spec", [WW(10, 3), RNN(8, 2)], ids=sid)
def test_wave_shapes_keep_the_op_sequence(spec):
    assert _lib.train_form(spec, device=True) == "wave"
    assert _lib.train_form(spec, device=False) == "lane"
    assert _lib.supports(spec, _lib.OP_RUN_MIXED, device=True)
    W, uid = population(spec, n=65, device=DEV)
    Wa, Wb = W.clone(), W.clone()
    fused, train = _lib.op_calls[_lib.OP_RUN_MIXED], _lib.op_calls[_lib.OP_TRAIN]
    ra = K.run_mixed(spec, Wa, 1, 2, EPS, uid=uid, seed=SEED, ctr=CTR)
    assert _lib.op_calls[_lib.OP_RUN_MIXED] == fused and _lib.op_calls[_lib.OP_TRAIN] > train
    rb = K.run_mixed_fused(spec, Wb, 1, 2, EPS, uid=uid, seed=SEED, ctr=CTR)  # the lane engine
    assert _lib.op_calls[_lib.OP_RUN_MIXED] == fused + 1
    assert int(ra[1].max()) >= 1  # some row performed a step
    assert_same((Wa, ra), (Wb, rb))


def test_lane_shapes_take_the_fused_launch():
    for spec in (WW(2, 2), AGG(4, 2, 2), RNN(2, 2), AGG(4, 4, 3)):
        assert _lib.train_form(spec, device=True) == "lane", spec
    W, uid = population(WW(2, 2), device=DEV)
    fused = _lib.op_calls[_lib.OP_RUN_MIXED]
    K.run_mixed(WW(2, 2), W, 1, 2, EPS, uid=uid)
    assert _lib.op_calls[_lib.OP_RUN_MIXED] == fused + 1


def test_long_training_steps_take_the_op_sequence():
    """the measured rule (profiles/mixed_run.md): the lane shapes leave the fused launch from an epoch
    count on, where few lanes of a wave would train for long; the result is the same bits"""
    assert [_lib.mixed_form(WW(2, 2), True, t) for t in (0, 50, 500)] == ["fused", "fused", "ops"]
    assert [_lib.mixed_form(RNN(2, 2), True, t) for t in (0, 50, 500)] == ["fused", "ops", "ops"]
    assert [_lib.mixed_form(AGG(4, 2, 2), True, t) for t in (0, 50, 500)] == ["fused"] * 3
    assert _lib.mixed_form(WW(10, 3), True, 0) == "ops"
    spec = RNN(2, 2)
    W, uid = population(spec, n=65, device=DEV)
    Wa, Wb = W.clone(), W.clone()
    fused = _lib.op_calls[_lib.OP_RUN_MIXED]
    ra = K.run_mixed(spec, Wa, 40, 2, EPS, uid=uid, seed=SEED, ctr=CTR)
    assert _lib.op_calls[_lib.OP_RUN_MIXED] == fused
    rb = K.run_mixed_fused(spec, Wb, 40, 2, EPS, uid=uid, seed=SEED, ctr=CTR)
    assert_same((Wa, ra), (Wb, rb))


def test_experiment_on_device_population():
    spec, n = WW(2, 2), 200
    out = {}
    for dev in ("cpu", DEV):
        exp = MixedFixpointExperiment()
        pop = Population(spec, n, device=dev, seed=9)
        out[dev] = exp.run_population(pop, trains_per_application=3, step_limit=STEPS, record=True)
        assert sum(exp.counters.values()) == n and len(exp.historical_particles) == n
        out[dev + "W"] = pop.W.cpu()
    assert out["cpu"] == out[DEV]
    assert torch.equal(bits(out["cpuW"]), bits(out[DEV + "W"]))
