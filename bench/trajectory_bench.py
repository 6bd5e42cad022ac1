#!/usr/bin/env python
"""Cost of recording self-application trajectories on one GPU (device events around synchronised
work, warm-up first, the variants alternated within each repetition; medians).

Aggregating(4,10,3), n particles x steps, early_exit=False:
  plain        record=False
  state        record="state"   (chunk states, steps * n * A * 4 bytes)
  dense        record=True      (rows, (steps + 1) * n * PP * 4 bytes)
  generic      record=True on the runtime-shape engine (force_generic): the only recording route
               before the chunk-state kernels recorded
Weightwise(16,2), n particles x steps:
  plain        record=False
  dense        record=True
  stepwise     one K.apply per step + a copy into the trajectory: the only recording route before
               the MFMA kernel recorded
Prints one JSON line per net: times (ms) and the achieved write bandwidth of the recorded bytes
(computed from the shapes; the dense figures include zero-filling the buffer, which every caller
pays).  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from self_replicating_neural_networks_amd.arch import ArchSpec  # noqa: E402
from self_replicating_neural_networks_amd.ops import _lib, kernels as K  # noqa: E402


def time_variants(variants, W, W0, reps, warmup):
    """median ms of each variant: every repetition runs all of them in turn (W restored before each,
    outside the timed region)"""
    ts = {k: [] for k in variants}
    for it in range(warmup + reps):
        for name, fn in variants.items():
            W.copy_(W0)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            del out
            if it >= warmup:
                ts[name].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def rows(spec, n, dev):
    W = torch.zeros(n, spec.PP, device=dev)
    K.init_rows(spec, W, torch.arange(n, dtype=torch.int64, device=dev), 1)
    return W


def forced_generic(fn):
    _lib.set_force_generic(True)
    try:
        return fn()
    finally:
        _lib.set_force_generic(False)


def bench_agg(dev, n, steps, reps, warmup):
    spec = ArchSpec.aggregating(4, 10, 3)
    W0 = rows(spec, n, dev)
    W = W0.clone()
    run = lambda record: K.run_fixpoint(spec, W, steps, 1e-4, early_exit=False, with_sec=False, record=record)  # noqa: E731
    t = time_variants({"plain": lambda: run(False), "state": lambda: run("state"), "dense": lambda: run(True),
                       "generic": lambda: forced_generic(lambda: run(True))}, W, W0, reps, warmup)
    dense_b, state_b = (steps + 1) * n * spec.PP * 4, steps * n * spec.aggregates * 4
    return {"arch": "aggregating(4,10,3)", "n": n, "steps": steps, "ms": t,
            "dense_bytes": dense_b, "state_bytes": state_b,
            "dense_write_GBps": dense_b / (t["dense"] * 1e-3) / 1e9,
            "generic_write_GBps": dense_b / (t["generic"] * 1e-3) / 1e9,
            "state_write_GBps": state_b / (t["state"] * 1e-3) / 1e9,
            "state_over_plain_ms": t["state"] - t["plain"],
            "dense_vs_generic": t["generic"] / t["dense"], "state_vs_generic": t["generic"] / t["state"]}


def bench_wide(dev, n, steps, reps, warmup):
    spec = ArchSpec.weightwise(16, 2)
    W0 = rows(spec, n, dev)
    W = W0.clone()
    run = lambda record: K.run_fixpoint(spec, W, steps, 1e-4, early_exit=False, with_sec=False, record=record)  # noqa: E731

    def stepwise():
        traj = torch.zeros((steps + 1, n, spec.PP), device=dev)
        traj[0].copy_(W)
        out = torch.empty_like(W)
        for s in range(steps):
            K.apply(spec, traj[s], out)
            traj[s + 1].copy_(out)
        W.copy_(out)
        return traj
    t = time_variants({"plain": lambda: run(False), "dense": lambda: run(True), "stepwise": stepwise}, W, W0, reps, warmup)
    dense_b = (steps + 1) * n * spec.PP * 4
    return {"arch": "weightwise(16,2)", "n": n, "steps": steps, "ms": t, "dense_bytes": dense_b,
            "dense_write_GBps": dense_b / (t["dense"] * 1e-3) / 1e9,
            "stepwise_write_GBps": dense_b / (t["stepwise"] * 1e-3) / 1e9,
            "dense_vs_stepwise": t["stepwise"] / t["dense"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agg-n", type=int, default=100_000)
    ap.add_argument("--wide-n", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trajectory_bench needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    res = []
    if args.agg_n:
        res.append(bench_agg(dev, args.agg_n, args.steps, args.reps, args.warmup))
        print(json.dumps(res[-1]), flush=True)
    if args.wide_n:
        res.append(bench_wide(dev, args.wide_n, args.steps, args.reps, args.warmup))
        print(json.dumps(res[-1]), flush=True)
    return res


if __name__ == "__main__":
    main()
