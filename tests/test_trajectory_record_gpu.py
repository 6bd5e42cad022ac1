"""Trajectory recording of run_fixpoint on the device for the nets the specialised kernels serve:
the chunk-state kernels of the big aggregating nets (dense and compact form), the MFMA weightwise
nets, the wave kernel of wide Recurrent nets, the tables the runtime-shape engine serves, and
run_population on top."""
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.experiment import FixpointExperiment
from self_replicating_neural_networks_amd.ops import _lib, kernels as K
from self_replicating_neural_networks_amd.population import Population
from test_trajectory_record import (AGG, EPS, N, STEPS, check_history, exercises_early_exit, make_rows, same,
                                    stepwise_chain)

pytestmark = pytest.mark.gpu

AGG82 = ArchSpec.aggregating(4, 8, 2)
WIDE = [ArchSpec.weightwise(16, 2), ArchSpec.weightwise(16, 3), ArchSpec.weightwise(32, 2)]
RNN = ArchSpec.recurrent(8, 2)
ids = lambda s: f"{s.kind[:3]}{s.width}_{s.depth}"  # noqa: E731


def _run(spec, W0, early_exit, record, steps=STEPS, **kw):
    W = W0.clone()
    cls, nsteps, traj = K.run_fixpoint(spec, W, steps, EPS, early_exit=early_exit, record=record, **kw)
    return W, cls, nsteps, traj


def _knob(name, value, fn):
    _lib.set_knob(name, value)
    try:
        return fn()
    finally:
        _lib.set_knob(name, -1)


def _forced_generic(fn):
    _lib.set_force_generic(True)
    try:
        return fn()
    finally:
        _lib.set_force_generic(False)


def _assert_runs_equal(a, b):
    for x, y, what in zip(a, b, ("W", "cls", "nsteps", "trajectory")):
        assert same(x, y) if x.is_floating_point() else torch.equal(x, y), what


@pytest.fixture(scope="module")
def agg_generic(cuda):
    """(W, cls, nsteps, dense trajectory) of Aggregating(4,10,3) on the runtime-shape engine, per early_exit:
    the reference of the specialised recordings, computed once"""
    W0 = make_rows(AGG, device=cuda)
    return {ee: _forced_generic(lambda: _run(AGG, W0, ee, True)) for ee in (True, False)}


@pytest.mark.parametrize("early_exit", [True, False])
@pytest.mark.parametrize("big_wave", [0, 1], ids=["row", "wave"])
def test_big_aggregating_dense_equals_generic(cuda, agg_generic, big_wave, early_exit):
    assert not _lib.is_generic(AGG, _lib.OP_RUN_FIXPOINT)
    W0 = make_rows(AGG, device=cuda)
    got = _knob("big_wave", big_wave, lambda: _run(AGG, W0, early_exit, True))
    ref = agg_generic[early_exit]
    if early_exit:
        assert exercises_early_exit(got[2])
    assert same(got[3][0], W0)
    _assert_runs_equal(got, ref)
    past = torch.arange(STEPS + 1, device=cuda)[:, None] > got[2][None, :]
    assert not got[3][past].any()  # zero rows after a particle's last step


def test_chunk_states_that_underflow_keep_the_row_arithmetic(cuda):
    """without early exit the states underflow to signed zeros; the mean of a chunk of -0 is +0 on the
    rows, so it is on the chunk states (no recording involved)"""
    W0 = make_rows(AGG, device=cuda)
    got = _run(AGG, W0, False, False, steps=12)
    ref = _forced_generic(lambda: _run(AGG, W0, False, False, steps=12))
    assert (got[0] == 0).all(dim=1).sum() > N // 2  # most rows ended at (signed) zero
    _assert_runs_equal(got[:3], ref[:3])


@pytest.mark.parametrize("early_exit", [True, False])
def test_big_aggregating_4_8_2_dense_equals_generic(cuda, early_exit):
    assert not _lib.is_generic(AGG82, _lib.OP_RUN_FIXPOINT)
    W0 = make_rows(AGG82, device=cuda)
    got = _run(AGG82, W0, early_exit, True)
    ref = _forced_generic(lambda: _run(AGG82, W0, early_exit, True))
    if early_exit:
        assert exercises_early_exit(got[2])
    _assert_runs_equal(got, ref)


@pytest.mark.parametrize("early_exit", [True, False])
@pytest.mark.parametrize("big_wave", [0, 1], ids=["row", "wave"])
def test_big_aggregating_state_form(cuda, agg_generic, big_wave, early_exit):
    W0 = make_rows(AGG, device=cuda)
    W, cls, nsteps, st = _knob("big_wave", big_wave, lambda: _run(AGG, W0, early_exit, "state"))
    Wr, cls_r, nsteps_r, dense = agg_generic[early_exit]
    if early_exit:
        assert exercises_early_exit(nsteps)
    assert isinstance(st, K.StateTrajectory) and st.states.shape == (STEPS, N, 4) and st.states.dtype == torch.float32
    assert same(W, Wr) and torch.equal(cls, cls_r) and torch.equal(nsteps, nsteps_r) and torch.equal(st.nsteps, nsteps_r)
    assert same(st.row0, W0)
    assert same(st.full(), dense)
    starts = [c[0] for c in AGG.chunks]
    assert same(st.states, dense[1:, :, starts])
    past = torch.arange(1, STEPS + 1, device=cuda)[:, None] > nsteps[None, :]
    assert not st.states[past].view(torch.int32).any()  # entries past nsteps are zero (bits)
    assert same(st.rows(2), dense[2])
    assert same(torch.from_numpy(st.particle(100)), dense[:int(nsteps[100]) + 1, 100, :AGG.P].cpu())


@pytest.mark.parametrize("spec", WIDE, ids=ids)
@pytest.mark.parametrize("early_exit", [True, False])
def test_mfma_weightwise_records_every_apply(cuda, spec, early_exit):
    assert not _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT)
    W0 = make_rows(spec, device=cuda)
    W, cls, nsteps, traj = _run(spec, W0, early_exit, True)
    if early_exit:
        assert exercises_early_exit(nsteps)
    assert traj.shape == (STEPS + 1, N, spec.PP) and same(traj[0], W0)
    out = torch.zeros_like(W0)
    for s in range(STEPS):
        K.apply(spec, traj[s].contiguous(), out)  # identity indices: out[p] = f_p(p)
        taken = s < nsteps
        assert same(traj[s + 1][taken], out[taken]), s
        assert not traj[s + 1][~taken].view(torch.int32).any(), s
    assert same(traj[nsteps.long(), torch.arange(N, device=cuda)], W)
    Wn, cls_n, nsteps_n, none = _run(spec, W0, early_exit, False)
    assert none is None and same(Wn, W) and torch.equal(cls_n, cls) and torch.equal(nsteps_n, nsteps)


@pytest.mark.parametrize("early_exit", [True, False])
def test_recurrent_wave_recording_equals_lane(cuda, early_exit):
    W0 = make_rows(RNN, device=cuda)
    wave = _knob("rnn_wave", 1, lambda: _run(RNN, W0, early_exit, True))
    lane = _knob("rnn_wave", 0, lambda: _run(RNN, W0, early_exit, True))
    if early_exit:
        assert exercises_early_exit(wave[2])
    _assert_runs_equal(wave, lane)
    plain = _knob("rnn_wave", 1, lambda: _run(RNN, W0, early_exit, False))
    assert plain[3] is None
    _assert_runs_equal(plain[:3], wave[:3])


@pytest.mark.parametrize("spec", [AGG, AGG82] + WIDE + [RNN], ids=ids)
def test_recording_changes_nothing_else(cuda, spec):
    W0 = make_rows(spec, device=cuda)
    plain = _run(spec, W0, True, False)
    assert plain[3] is None and exercises_early_exit(plain[2])
    forms = [True] + (["state"] if spec.kind == "aggregating" else [])
    for record in forms:
        _assert_runs_equal(_run(spec, W0, True, record)[:3], plain[:3])
    if spec.kind != "aggregating":
        with pytest.raises(ValueError, match="state"):
            _run(spec, W0, True, "state")


@pytest.mark.parametrize("spec", [AGG, AGG82] + WIDE + [RNN], ids=ids)
def test_single_row(cuda, spec):
    W0 = make_rows(spec, device=cuda)[100:101].contiguous()
    W, cls, nsteps, traj = _run(spec, W0, True, True)
    ref = _forced_generic(lambda: _run(spec, W0, True, True))
    assert int(nsteps[0]) > 0
    _assert_runs_equal((W, cls, nsteps, traj), ref)
    if spec.kind == "aggregating":
        Ws, _, _, st = _run(spec, W0, True, "state")
        assert same(st.full(), traj) and same(Ws, W)


@pytest.mark.parametrize("case", ["bf16", "shuffle"])
@pytest.mark.parametrize("early_exit", [True, False])
def test_big_aggregating_tables_of_the_runtime_shape_engine(cuda, case, early_exit):
    """bf16 tables and shuffled nets run on the runtime-shape engine; their recording is the chain of
    one-step launches (16-bit: a float32 step rounded to the storage format)"""
    spec = ArchSpec.aggregating(4, 10, 3, shuffler="random") if case == "shuffle" else AGG
    dtype = torch.bfloat16 if case == "bf16" else torch.float32
    assert _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT, K.dtype_code(dtype))
    W0 = make_rows(spec, device=cuda, dtype=dtype)
    uid = torch.arange(N, dtype=torch.int64, device=cuda) + 3
    W, cls, nsteps, traj = _run(spec, W0, early_exit, True, uid=uid, seed=9, ctr=4)
    if early_exit:
        assert exercises_early_exit(nsteps)
    ref, last, ref_steps = stepwise_chain(spec, W0, STEPS, EPS, early_exit, uid=uid, seed=9, ctr=4, via_float=True)
    assert torch.equal(nsteps, ref_steps)
    assert same(traj, ref) and same(W, last)


def test_run_population_on_the_device(cuda):
    rows = make_rows(AGG, device=cuda)
    W0 = torch.cat([rows[[0, 8, 12]], rows[16:28], rows[80:90], rows[140:150], rows[300:305]])
    assert W0.shape[0] == 40
    pop = Population(AGG, 40, device=cuda, weights=W0, uid_start=7)
    ref = W0.clone()
    _, nsteps, dense = K.run_fixpoint(AGG, ref, STEPS, EPS, record=True)
    assert exercises_early_exit(nsteps)
    exp = FixpointExperiment()
    counts = exp.run_population(pop, STEPS, record=True)
    assert sum(counts.values()) == 40 and same(pop.W, ref)
    assert sorted(exp.historical_particles) == list(range(7, 47))
    check_history(exp, pop, dense, nsteps)
