"""Wide / long Recurrent nets wave per particle (csrc/srnn_generic.hip k_rnn_wave):
equal to the lane-per-particle path on the same device (same operation order) and close to
the host path, for self-application, run_fixpoint + census, self-training and learn_from.

From the init rows no row of these nets is finite after two self-applications or three BPTT
epochs, so every comparison runs a second time from the rows scaled by 0.5 (HALF), where every
row stays finite through all of ``_ops`` and the soups (checked on the host path); there at least
90 % of the lane path's rows must be finite in every compared float output.  The kernels are pinned to the exact
oracle directly in tests/test_exact_families_gpu.py."""
import numpy as np
import pytest
import torch

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.ops import kernels as K
from self_replicating_neural_networks_amd.population import Population

pytestmark = pytest.mark.gpu


HALF = 0.5


def _finite_share(t):
    return float(torch.isfinite(t.float().reshape(t.shape[0], -1)).all(dim=1).float().mean())


def _ops(spec, dev, n=300, scale=1.0):
    pop = Population(spec, n, device=dev, seed=4)
    pop.W.mul_(scale)
    W0 = pop.W.clone()
    out = {}
    pop.self_apply(2)
    out["apply"] = pop.W.clone()
    pop.W.copy_(W0)
    cls, steps, _ = K.run_fixpoint(spec, pop.W, 4, 1e-4, early_exit=True)
    out["fix"], out["cls"], out["steps"] = pop.W.clone(), cls.clone(), steps.clone()
    pop.W.copy_(W0)
    out["loss"] = pop.train(3).clone()
    out["train"] = pop.W.clone()
    pop.W.copy_(W0)
    idx = torch.roll(torch.arange(n, device=dev), 3).contiguous()
    pop.learn_from(W0.clone(), idx, epochs=2)
    out["learn"] = pop.W.clone()
    torch.cuda.synchronize() if dev != "cpu" else None
    return out


@pytest.mark.parametrize("w,d", [(8, 2), (16, 2), (12, 3)])
def test_rnn_wave_equals_lane_path(cuda, w, d):
    spec = ArchSpec.recurrent(w, d)
    for scale in (1.0, HALF):
        outs = []
        for wave in (True, False):
            _lib.set_rnn_wave(wave)
            try:
                outs.append(_ops(spec, cuda, scale=scale))
            finally:
                _lib.set_rnn_wave(True)
        a, b = outs
        for k in a:
            x, y = a[k], b[k]
            if x.is_floating_point():
                assert scale == 1.0 or _finite_share(y) >= 0.9, k
                assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32)
                                   if y.dtype == torch.float32 else y), (k, scale)
            else:
                assert torch.equal(x, y), (k, scale)
        h = _ops(spec, "cpu", scale=scale)
        ok = torch.isfinite(h["apply"]).all(1)
        assert scale == 1.0 or float(ok.float().mean()) >= 0.9
        assert torch.isfinite(a["apply"].cpu()[ok]).all()
        assert torch.allclose(a["apply"].cpu()[ok], h["apply"][ok], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("w,d", [(8, 2), (16, 2), (32, 2), (8, 3), (16, 3)])
def test_rnn_wave_specialised_equals_runtime_shape(cuda, w, d):
    """The width / depth-specialised wave kernels (compile-time layer tables, unrolled loops)
    are bitwise the runtime-shape wave kernel."""
    spec = ArchSpec.recurrent(w, d)
    for scale in (1.0, HALF):
        outs = []
        for on in (True, False):
            _lib.set_rnn_spec(on)
            try:
                outs.append(_ops(spec, cuda, n=200, scale=scale))
            finally:
                _lib.set_rnn_spec(True)
        a, b = outs
        for k in a:
            x, y = a[k], b[k]
            if x.dtype == torch.float32:
                assert scale == 1.0 or _finite_share(y) >= 0.9, k
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), (k, scale)


SOUP = dict(attacking_rate=0.2, learn_from_rate=0.2, train=2, learn_from_severity=2, remove_divergent=True,
            remove_zero=True, epsilon=1e-4)


def _soup(spec, dev, dtype, graphs, scale=1.0):
    from self_replicating_neural_networks_amd.soup_engine import SoupEngine

    rows0 = None
    if scale != 1.0:
        rows0 = SoupEngine(spec, 150, SOUP, device=dev, seed=13, dtype=dtype).local_rows()[:, :spec.P].float().cpu() * scale
    e = SoupEngine(spec, 150, SOUP, device=dev, seed=13, dtype=dtype, weights=rows0)
    e.stats = True
    if graphs:
        assert e.capture(warmup=1)
        e.evolve(2)
    else:
        e.evolve(3)
    torch.cuda.synchronize()
    return (e.local_rows().clone(), e.uid.clone(), e.loss.clone(), e.action.clone(), e.counterpart.clone(),
            e.respawn.clone(), e.last_census(), int(e.next_uid))


def _wave_and_lane_soups(spec, cuda, dtype, scale):
    """the same soup on the wave kernel and on the lane path: every output equal bitwise; from the
    half-scale rows at least 90 % of the lane path's rows and losses are finite (100 % and 94 % on
    the host path), so the second learn_from / self-train epoch is compared on numbers"""
    bits = lambda t: t.contiguous().view(torch.uint8) if t.is_floating_point() else t
    outs = []
    for wave in (True, False):
        _lib.set_rnn_soup(wave)
        try:
            outs.append(_soup(spec, cuda, dtype, graphs=False, scale=scale))
        finally:
            _lib.set_rnn_soup(True)
    a, b = outs
    for k, (x, y) in enumerate(zip(a[:6], b[:6])):
        if x.is_floating_point():
            assert scale == 1.0 or _finite_share(y) >= 0.9, (k, scale)
        assert torch.equal(bits(x), bits(y)), (k, scale)
    assert a[6:] == b[6:]
    assert int((a[3] == 3).sum()) > 0  # self-training happened
    return a


@pytest.mark.parametrize("w,d", [(8, 2), (12, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_rnn_wave_soup_equals_lane_path(cuda, w, d, dtype):
    """Recurrent soup generations wave per particle (k_rnn_wave_soup: attacks, learn_from,
    self-train, respawn with inline re-init) == the lane path, bitwise, from the half-scale rows
    and from the init rows; graphs == eager"""
    spec = ArchSpec.recurrent(w, d)
    bits = lambda t: t.contiguous().view(torch.uint8) if t.is_floating_point() else t
    _wave_and_lane_soups(spec, cuda, dtype, HALF)
    a = _wave_and_lane_soups(spec, cuda, dtype, 1.0)
    g = _soup(spec, cuda, dtype, graphs=True)
    for k, (x, y) in enumerate(zip(g[:6], a[:6])):
        assert torch.equal(bits(x), bits(y)), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_rnn_wave_soup_runtime_shape_from_half_scale_rows(cuda, dtype):
    """the runtime-shape instantiation k_rnn_wave_soup<0,0> (what RNN(12,3) runs) also on RNN(8,2), with the
    specialisations off (the soup launch goes through rw_launch, which reads the knob) == the lane path
    on finite rows"""
    spec = ArchSpec.recurrent(8, 2)
    _lib.set_rnn_spec(False)
    try:
        assert _lib.get_knob("rnn_spec") == 0 and _lib.get_knob("rnn_soup") != 0 and _lib.get_knob("rnn_wave") != 0
        _wave_and_lane_soups(spec, cuda, dtype, HALF)
    finally:
        _lib.set_rnn_spec(True)
