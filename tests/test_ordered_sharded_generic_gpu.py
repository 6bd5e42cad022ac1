"""The sharded reference-order generation of the runtime shapes (csrc/srnn_generic.hip
g_soup_ordered_sh) on the device: 2 and 3 ranks on the one-GPU box (gloo process group, every rank on
cuda:0, the all-gathers staged through the host, at most 3 children at a time) must reproduce the
single-rank device reference-order soup of the same shape -- itself pinned to the serial loop and the
exact oracle -- bitwise, in each form of the level launch: a lane per turn (k_gordsh_level), a group
of lanes per turn (k_gordsh_level_ww) and a wave per turn (k_gordsh_level_rnn).  Every rank asserts
the form it runs, so a silent fallback to the lane form cannot pass (the device counterpart of
tests/test_ordered_sharded_generic.py; the pattern of tests/test_ordered_sharded_gpu.py)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from self_replicating_neural_networks_amd.arch import ArchSpec
from self_replicating_neural_networks_amd.ops import _lib
from self_replicating_neural_networks_amd.parallel.dist import Dist
from self_replicating_neural_networks_amd.soup_engine import SoupEngine, engine_bytes

pytestmark = pytest.mark.gpu

PARAMS = dict(attacking_rate=0.2, learn_from_rate=0.2, train=3, learn_from_severity=1, remove_divergent=True,
              remove_zero=True, epsilon=1e-4)
N_TOTAL, SEED = 1003, 21
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, spec_json, dtype, chunks, ord_wave, form):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SRNN_SHARE_DEVICE="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        if not ord_wave:
            _lib.set_knob("ord_wave", 0)
        e = SoupEngine(ArchSpec.from_json(spec_json), N_TOTAL, PARAMS, device=dev, seed=SEED,
                       dist=Dist(rank, world, 0, None), dtype=DTYPES[dtype], order="sequential")
        assert e.ordered_sharded_form() == form and e.ordered_run_form() is None
        assert e._scratch.numel() >= _lib.generic_ordsh_scratch_bytes(e.spec, e.n, e.dtype_code)
        e.stats = True
        for k in chunks:
            e.evolve(k)
        assert e.ordered_sharded_form() == form
        counts = e.count()
        census = e.last_census()  # (the last generation's own census, all ranks' rows)
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), W=e.local_rows().float().cpu().numpy(),
                 uid=e.uid.cpu().numpy(), next_uid=e.next_uid.cpu().numpy(), loss=e.loss.cpu().numpy(),
                 counts=np.array([counts[k] for k in sorted(counts)]),
                 census=np.array([census[k] for k in sorted(census)]), err=np.array([e.ordered_error()]))
    finally:
        dist.destroy_process_group()


# shape, ranks, dtype, chunks, knob ord_wave, the form every rank must report
CASES = [
    ("ww-10-3-group", ArchSpec.weightwise(10, 3), 2, "float32", (3,), True, "wave"),   # U = 16, G = 4
    ("ww-3-3-group", ArchSpec.weightwise(3, 3), 3, "float32", (1, 2), True, "wave"),   # U = 4, G = 16
    ("rnn-8-2-wave", ArchSpec.recurrent(8, 2), 2, "float32", (3,), True, "wave"),
    ("agg-4-4-3-lane", ArchSpec.aggregating(4, 4, 3), 2, "float32", (3,), True, "lane"),
    ("ww-3-3-lane", ArchSpec.weightwise(3, 3), 2, "float32", (3,), False, "lane"),     # a group shape, knob off
    ("ww-10-3-bf16", ArchSpec.weightwise(10, 3), 2, "bfloat16", (3,), True, "wave"),
    # an MFMA-family shape: its census kernel (k_wide) counts classes only, so the classify that closes a
    # generation of the all-gather exchange -- respawn count, generation counter -- must be the runtime-shape one
    ("ww-16-2-group", ArchSpec.weightwise(16, 2), 2, "float32", (1, 2), True, "wave"),
]


@pytest.mark.parametrize("spec,world,dtype,chunks,ord_wave,form", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_device_sharded_reference_order_of_a_runtime_shape_equals_single_rank(tmp_path, spec, world, dtype, chunks,
                                                                              ord_wave, form):
    ref = SoupEngine(spec, N_TOTAL, PARAMS, device="cuda", seed=SEED, dtype=DTYPES[dtype], order="sequential")
    assert ref._ord_generic
    ref.evolve(sum(chunks))
    ref_counts = ref.count()
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path), spec.to_json(), dtype, chunks, ord_wave, form),
                       nprocs=world, start_method="spawn", join=True)
    parts = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]
    W = np.concatenate([p["W"] for p in parts])
    assert np.array_equal(np.concatenate([p["uid"] for p in parts]), ref.uid.cpu().numpy())
    assert np.array_equal(W.view(np.int32), ref.local_rows().float().cpu().numpy().view(np.int32))
    assert np.array_equal(np.concatenate([p["loss"] for p in parts]).view(np.int32),
                          ref.loss.cpu().numpy().view(np.int32))
    for p in parts:
        assert int(p["next_uid"][0]) == int(ref.next_uid[0]) and int(p["err"][0]) == 0
        assert list(p["counts"]) == [ref_counts[k] for k in sorted(ref_counts)]
        # the generation's own census (stats = True) == the classify kernel on the single-rank soup's rows
        assert list(p["census"]) == [ref_counts[k] for k in sorted(ref_counts)]
        assert int(p["census"].sum()) == N_TOTAL


def _held_bytes(e: SoupEngine) -> int:
    seen, total = set(), 0
    for t in e._state() + [e._scratch]:
        if t is None or t.data_ptr() in seen:
            continue
        seen.add(t.data_ptr())
        total += t.numel() * t.element_size()
    return total


def test_engine_bytes_of_a_device_rank_counts_the_level_scratch():
    """one of 8 ranks of WW(10,3) on the device (no process group, no generation run): the estimate
    against the tensors it holds, the scratch of its level and close launches included, with the
    bounds of tests/test_exec_config.py"""
    spec, n, world = ArchSpec.weightwise(10, 3), 5003, 8
    from self_replicating_neural_networks_amd.config import ExecConfig
    # (no communicator of its own: without a process group there is no backend to ask for one)
    d = Dist(world=world, rank=3, execution=ExecConfig(native_comm=False))
    e = SoupEngine(spec, n, dict(train=1), device="cuda", dist=d, order="sequential")
    assert e.ordered_sharded_form() == "wave" and e._scratch is not None
    assert e._scratch.numel() >= _lib.generic_ordsh_scratch_bytes(spec, e.n)
    est = engine_bytes(spec, n, world=world, order="sequential", epochs=2)
    held = _held_bytes(e)
    assert est >= held * 0.99 and est <= held * 1.05 + 512, (est, held)
