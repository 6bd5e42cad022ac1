"""The wave run of reference-order generations of the wide Recurrent nets (csrc/srnn_generic.hip
k_gord_run_rnn: a wave per turn), host side: which shapes the run-form query gives it to, and the
knobs that take it away (SRNN_KNOB_ORD_WAVE, SRNN_KNOB_RNN_WAVE).  No GPU needed: the query is host
code, and on the host every shape's turn is a lane's (one thread's)."""
import pytest

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.ops import _lib

WIDE = [ArchSpec.recurrent(8, 2), ArchSpec.recurrent(16, 2), ArchSpec.recurrent(8, 3), ArchSpec.recurrent(12, 2)]
RNN82 = ArchSpec.recurrent(8, 2)


@pytest.fixture
def no_env(monkeypatch):
    for name in ("SRNN_ORD_WAVE", "SRNN_RNN_WAVE"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("spec", WIDE, ids=str)
def test_the_wave_run_serves_the_wide_recurrent_nets_on_the_device(spec, no_env):
    assert _lib.get_knob("ord_wave") == -1 and _lib.get_knob("rnn_wave") == -1
    assert _lib.ord_run_form(spec, dev=True) == "wave"
    for dc in (_lib.DTYPE_BF16, _lib.DTYPE_FP16):
        assert _lib.ord_run_form(spec, dev=True, dtype_code=dc) == "wave"


@pytest.mark.parametrize("spec", WIDE, ids=str)
def test_the_host_run_form_stays_the_lane(spec, no_env):
    assert _lib.ord_run_form(spec, dev=False) == "lane"


@pytest.mark.parametrize("spec", [ArchSpec.recurrent(3, 2), ArchSpec.recurrent(2, 2)], ids=str)
def test_narrow_recurrent_nets_stay_on_the_lane_run(spec, no_env):
    assert _lib.ord_run_form(spec, dev=True) == "lane"


@pytest.mark.parametrize("knob", ["ord_wave", "rnn_wave"])
def test_either_knob_off_gives_the_lane_run(knob, no_env):
    try:
        _lib.set_knob(knob, 0)
        assert _lib.ord_run_form(RNN82, dev=True) == "lane"
        _lib.set_knob(knob, 1)
        assert _lib.ord_run_form(RNN82, dev=True) == "wave"
    finally:
        _lib.set_knob(knob, -1)
    assert _lib.ord_run_form(RNN82, dev=True) == "wave"


def test_the_environment_variable_wins_over_the_knob(no_env):
    try:
        _lib.set_knob("ord_wave", 1)
        no_env.setenv("SRNN_ORD_WAVE", "0")
        assert _lib.ord_run_form(RNN82, dev=True) == "lane"
        _lib.set_knob("ord_wave", 0)
        no_env.setenv("SRNN_ORD_WAVE", "1")
        assert _lib.ord_run_form(RNN82, dev=True) == "wave"
    finally:
        _lib.set_knob("ord_wave", -1)
