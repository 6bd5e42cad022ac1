"""The group run of reference-order generations (csrc/srnn_generic.hip k_gord_run_ww), host side: its
knob (SRNN_KNOB_ORD_WAVE / SRNN_ORD_WAVE / ExecConfig.ord_wave) and the run-form query.  No GPU
needed: on the host every shape's turn is a lane's (one thread's)."""
import pytest

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.config import ExecConfig
from self_replicating_neural_networks_amd.ops import _lib

SHAPES = [ArchSpec.weightwise(2, 2), ArchSpec.weightwise(3, 3), ArchSpec.weightwise(5, 2), ArchSpec.weightwise(10, 3),
          ArchSpec.weightwise(16, 2), ArchSpec.aggregating(4, 2, 2), ArchSpec.aggregating(4, 4, 3),
          ArchSpec.recurrent(2, 2), ArchSpec.recurrent(3, 2), ArchSpec.fft(3, 2, 2)]


def test_knob_is_a_library_knob_and_an_exec_config_field():
    assert _lib.KNOBS["ord_wave"] == 12 and _lib.KNOB_ENV["ord_wave"] == "SRNN_ORD_WAVE"
    assert set(_lib.KNOBS) == set(ExecConfig.LIBRARY_KNOBS)
    assert "ord_wave" in ExecConfig.TRI_STATE and ExecConfig._ENV["ord_wave"] == "SRNN_ORD_WAVE"
    assert ExecConfig().ord_wave is None


def test_knob_round_trip_through_config_library_and_environment(monkeypatch):
    monkeypatch.delenv("SRNN_ORD_WAVE", raising=False)
    assert _lib.get_knob("ord_wave") == -1  # the built-in default (on)
    try:
        ExecConfig(ord_wave=False).apply_library()
        assert _lib.get_knob("ord_wave") == 0
        ExecConfig(ord_wave=True).apply_library()
        assert _lib.get_knob("ord_wave") == 1
        ExecConfig().apply_library()  # None: left as it is
        assert _lib.get_knob("ord_wave") == 1
        monkeypatch.setenv("SRNN_ORD_WAVE", "0")
        assert _lib.get_knob("ord_wave") == 0  # the environment variable wins
        assert ExecConfig(ord_wave=True).resolved().ord_wave is False
        assert ExecConfig().in_force()["library"]["ord_wave"] == 0
        monkeypatch.setenv("SRNN_ORD_WAVE", "1")
        assert ExecConfig().resolved().ord_wave is True and _lib.get_knob("ord_wave") == 1
        monkeypatch.delenv("SRNN_ORD_WAVE")
        assert ExecConfig().resolved().ord_wave is None
    finally:
        _lib.set_knob("ord_wave", -1)
    assert _lib.get_knob("ord_wave") == -1


@pytest.mark.parametrize("knob", [-1, 0, 1])
@pytest.mark.parametrize("spec", SHAPES, ids=str)
def test_host_run_form_is_the_lane_for_every_shape(spec, knob):
    try:
        _lib.set_knob("ord_wave", knob)
        assert _lib.ord_run_form(spec, dev=False) == "lane"
        for dc in (_lib.DTYPE_BF16, _lib.DTYPE_FP16):
            assert _lib.ord_run_form(spec, dev=False, dtype_code=dc) == "lane"
    finally:
        _lib.set_knob("ord_wave", -1)


def test_a_shape_without_a_host_generation_has_no_host_run_form():
    big = ArchSpec.aggregating(4, 10, 3)  # P = 280: device only
    assert not _lib.supports(big, _lib.OP_SOUP_ORDERED, False)
    assert _lib.ord_run_form(big, dev=False) is None


def test_device_run_form_query_follows_the_knob(monkeypatch):
    """(the query is host code: which kernel a device generation would launch)"""
    monkeypatch.delenv("SRNN_ORD_WAVE", raising=False)
    ww, rnn = ArchSpec.weightwise(3, 3), ArchSpec.recurrent(3, 2)
    try:
        assert _lib.ord_run_form(ww) == "wave" and _lib.ord_run_form(rnn) == "lane"
        assert _lib.ord_run_form(ArchSpec.weightwise(2, 2)) == "lane"  # a template shape
        _lib.set_knob("ord_wave", 0)
        assert _lib.ord_run_form(ww) == "lane"
        monkeypatch.setenv("SRNN_ORD_WAVE", "1")
        assert _lib.ord_run_form(ww) == "wave"
    finally:
        _lib.set_knob("ord_wave", -1)
