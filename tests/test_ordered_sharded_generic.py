"""The sharded reference-order generation of the runtime shapes (csrc/srnn_generic.hip
g_soup_ordered_sh: the level-synchronous protocol of csrc/srnn_ordered_sh.h with the runtime-shape
turn and close) on the host: every rank plans the whole generation, runs its own turns level by
level and all-gathers each level's outputs.  The result must be BITWISE the single-rank
reference-order engine of the same shape -- rows, uids, actions, losses, census -- for any rank count
(gloo on CPU, the pattern of tests/test_ordered_sharded.py; device ranks:
tests/test_ordered_sharded_generic_gpu.py)."""
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

HOT = dict(attacking_rate=0.3, learn_from_rate=0.3, train=2, learn_from_severity=2, remove_divergent=True,
           remove_zero=True, epsilon=1e-4)
BENCH = dict(attacking_rate=0.1, learn_from_rate=0.1, train=3, learn_from_severity=1, remove_divergent=True,
             remove_zero=True, epsilon=1e-4)
N_TOTAL, GENS = 307, 4  # uneven shards on purpose
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, spec_json, out_dir, params, dtype, chunks):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d = Dist(rank, world, 0, None, force=world == 1)
        e = SoupEngine(ArchSpec.from_json(spec_json), N_TOTAL, params, device="cpu", seed=13, dist=d,
                       dtype=DTYPES[dtype], order="sequential")
        assert e.ordered_sharded_form() == "lane" and e.ordered_run_form() is None
        e.stats = True
        for k in chunks:
            e.evolve(k)
        counts = e.count()
        lv = e.ordered_levels()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), W=e.local_rows().float().numpy(), uid=e.uid.numpy(),
                 next_uid=e.next_uid.numpy(), action=e.action.numpy(), loss=e.loss.numpy(),
                 respawn=e.respawn.numpy(), counts=np.array([counts[k] for k in sorted(counts)]),
                 max_level=np.array([lv["max_level"], lv["error"]]))
    finally:
        dist.destroy_process_group()


def _run(tmp_path, spec, world, params=HOT, dtype="float32", chunks=(GENS,)):
    ref = SoupEngine(spec, N_TOTAL, params, device="cpu", seed=13, dtype=DTYPES[dtype], order="sequential")
    ref.evolve(sum(chunks))
    ref_counts = ref.count()
    mp.start_processes(_worker, args=(world, _free_port(), spec.to_json(), str(tmp_path), params, dtype, chunks),
                       nprocs=world, start_method="spawn", join=True)
    parts = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]
    cat = {k: np.concatenate([p[k] for p in parts]) for k in ("W", "uid", "action", "loss", "respawn")}
    assert np.array_equal(cat["uid"], ref.uid.numpy())
    assert np.array_equal(cat["W"].view(np.int32), ref.local_rows().float().numpy().view(np.int32))
    assert np.array_equal(cat["action"], ref.action.numpy()) and np.array_equal(cat["respawn"], ref.respawn.numpy())
    assert np.array_equal(cat["loss"].view(np.int32), ref.loss.numpy().view(np.int32))
    for p in parts:
        assert int(p["next_uid"][0]) == int(ref.next_uid[0])
        assert list(p["counts"]) == [ref_counts[k] for k in sorted(ref_counts)]
        assert int(p["max_level"][1]) == 0 and int(p["max_level"][0]) >= 1


CASES = [
    ("ww-3-3-w3", ArchSpec.weightwise(3, 3), 3, (1, 3)),
    ("ww-3-3-w1", ArchSpec.weightwise(3, 3), 1, (1, 2, 1)),  # the forced one-rank group
    ("agg-4-4-3", ArchSpec.aggregating(4, 4, 3), 2, (GENS,)),
    ("rnn-3-2", ArchSpec.recurrent(3, 2), 2, (GENS,)),
    ("rnn-8-2", ArchSpec.recurrent(8, 2), 3, (GENS,)),
    ("fft-4-2-2", ArchSpec.fft(4, 2, 2), 2, (GENS,)),
]


@pytest.mark.parametrize("spec,world,chunks", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_sharded_reference_order_of_a_runtime_shape_equals_single_rank(tmp_path, spec, world, chunks):
    _run(tmp_path, spec, world, chunks=chunks)


def test_sharded_reference_order_of_a_runtime_shape_bench_params_bf16(tmp_path):
    _run(tmp_path, ArchSpec.weightwise(10, 3), 2, params=BENCH, dtype="bfloat16")


def test_the_runtime_shapes_are_served_but_the_big_aggregating_nets():
    for spec in [c[1] for c in CASES] + [ArchSpec.weightwise(10, 3), ArchSpec.weightwise(16, 2),
                                          ArchSpec.recurrent(16, 2)]:
        for dev in (False, True):
            assert _lib.supports(spec, _lib.OP_SOUP_ORDERED_SH, dev) == _lib.supports(spec, _lib.OP_SOUP_ORDERED, dev)
            assert _lib.supports(spec, _lib.OP_SOUP_ORDERED_SH, dev), (spec, dev)
    big = ArchSpec.aggregating(4, 10, 3)
    assert not _lib.supports(big, _lib.OP_SOUP_ORDERED_SH, False) and not _lib.supports(big, _lib.OP_SOUP_ORDERED_SH, True)
    assert _lib.ordsh_form(big) is None
    with pytest.raises(NotImplementedError, match="big aggregating"):
        SoupEngine(big, 64, dict(train=1), device="cpu", dist=Dist(world=2, rank=0), order="sequential")
    # the forms, with the knob in force (the device ones are asserted on running engines in the GPU file)
    assert _lib.ordsh_form(ArchSpec.weightwise(2, 2)) == "lane"  # a lane template
    assert _lib.ordsh_form(ArchSpec.weightwise(10, 3)) == "wave" and _lib.ordsh_form(ArchSpec.recurrent(8, 2)) == "wave"
    assert _lib.ordsh_form(ArchSpec.aggregating(4, 4, 3)) == "lane" and _lib.ordsh_form(ArchSpec.recurrent(3, 2)) == "lane"
    assert _lib.ordsh_form(ArchSpec.weightwise(10, 3), dev=False) == "lane"
    _lib.set_knob("ord_wave", 0)
    try:
        assert _lib.ordsh_form(ArchSpec.weightwise(10, 3)) == "lane" and _lib.ordsh_form(ArchSpec.recurrent(8, 2)) == "lane"
    finally:
        _lib.set_knob("ord_wave", -1)
    # the scratch of a rank grows with its own turns and covers the recurrent wave slices
    ww, rnn = ArchSpec.weightwise(3, 3), ArchSpec.recurrent(8, 2)
    assert _lib.generic_ordsh_scratch_bytes(ww, 1500) > _lib.generic_ordsh_scratch_bytes(ww, 100) > 0
    assert _lib.generic_ordsh_scratch_bytes(rnn, 640) >= 2048 + 640 * 4 + 640 * (rnn.P * (2 * 8 + 1) * 4 + 8 * 8 * 8)


def _held_bytes(e: SoupEngine) -> int:
    seen, total = set(), 0
    for t in e._state() + [e._scratch]:
        if t is None or t.data_ptr() in seen:
            continue
        seen.add(t.data_ptr())
        total += t.numel() * t.element_size()
    return total


def test_engine_bytes_of_a_sharded_reference_order_rank_of_a_runtime_shape():
    """the estimate against the tensors one of 8 ranks holds (no process group needed to construct it),
    with the bounds of tests/test_exec_config.py.  The scratch of the level and close launches is a
    device buffer a host engine does not hold (as the run scratch in tests/test_ordered_generic.py):
    what a device rank allocates for it is added to the held bytes"""
    spec, n, world = ArchSpec.weightwise(3, 3), 5003, 8
    e = SoupEngine(spec, n, dict(train=1), device="cpu", dist=Dist(world=world, rank=3), order="sequential")
    assert not e.x2 and not e._ord_pipe and e._scratch is None and e.ordered_sharded_form() == "lane"
    est = engine_bytes(spec, n, world=world, order="sequential", epochs=2)
    held = _held_bytes(e)
    own = -(-n // world)
    scratch = max(_lib.generic_scratch_bytes(spec, own), _lib.generic_ordsh_scratch_bytes(spec, own))
    assert scratch >= own * 4 * 4 * spec.PP  # at least four row vectors per lane of the level launch
    held += scratch
    assert est >= held * 0.99 and est <= held * 1.05 + 512, (est, held)
