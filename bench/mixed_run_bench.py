"""Mixed self-attack / self-train runs on the device: ms per run of three forms of the same work.

  fused   one OP_RUN_MIXED launch (``K.run_mixed_fused``)
  ops     the op sequence on compacted tables (``K.run_mixed_ops``)
  loop    the Python loop ``mixed_self_fixpoints`` used before the operator existed (every row
          trained in every step, stopped rows restored with ``torch.where``), kept here as the baseline

Weightwise(2,2), Aggregating(4,2,2) and Recurrent(2,2) run at the setup's K = 4 with T in {0, 50, 500}
and 100k rows, WW(10,3) and RNN(8,2) at 10k rows with T = 50.  Every shape and T is warmed up first;
the three forms then alternate ``--reps`` times in one process, each call between two device
synchronisations.  The spread of a shape is what the loop's repeats differ by.  ``picked`` is the
form ``K.run_mixed`` takes for the shape and T (``_lib.mixed_form``); ``equal`` says the fused table, the op
sequence's and the loop's are the same bits.  Needs a GPU: there is no host fallback.

    python bench/mixed_run_bench.py [--reps 2] [--rows 100000] [--wide-rows 10000]

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_STEPS, EPS, SEED = 4, 1e-4, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--wide-rows", type=int, default=10000)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("mixed_run_bench: no ROCm device (this benchmark measures the GPU only)")
    from self_replicating_neural_networks_amd.arch import ArchSpec
    from self_replicating_neural_networks_amd.ops import _lib
    from self_replicating_neural_networks_amd.ops import kernels as K
    from self_replicating_neural_networks_amd.population import Population

    dev = torch.device("cuda", 0)
    cases = [(name, spec, args.rows, t)
             for name, spec in (("ww22", ArchSpec.weightwise(2, 2)), ("agg422", ArchSpec.aggregating(4, 2, 2)),
                                ("rnn22", ArchSpec.recurrent(2, 2)))
             for t in (0, 50, 500)]
    cases += [("ww103", ArchSpec.weightwise(10, 3), args.wide_rows, 50),
              ("rnn82", ArchSpec.recurrent(8, 2), args.wide_rows, 50)]

    def fresh(spec, n):
        return Population(spec, n, device=dev, seed=SEED)

    def loop(pop, t):  # the setup's loop before OP_RUN_MIXED
        active = torch.ones(pop.n, dtype=torch.bool, device=pop.device)
        for _ in range(K_STEPS):
            before = pop.W.clone()
            pop.self_apply(1)
            if t:
                pop.train(t)
            pop.W.copy_(torch.where(active[:, None], pop.W, before))
            cls, _ = pop.classify(EPS, with_sec=False)
            active &= ~((cls == 0) | (cls == 1) | (cls == 2))
            if not bool(active.any()):
                break
        return pop.W

    def fused(pop, t):
        K.run_mixed_fused(pop.spec, pop.W, t, K_STEPS, EPS, check_first=False, lr=pop.lr, uid=pop.uid, seed=pop.seed)
        return pop.W

    def ops(pop, t):
        K.run_mixed_ops(pop.spec, pop.W, t, K_STEPS, EPS, check_first=False, lr=pop.lr, uid=pop.uid, seed=pop.seed)
        return pop.W

    forms = (("loop", loop), ("fused", fused), ("ops", ops))

    def timed(f, spec, n, t):
        pop = fresh(spec, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        W = f(pop, t)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, W

    for _, spec, n, t in cases:  # warm-up: every kernel of every shape and form
        for _, f in forms:
            timed(f, spec, n, t)

    results = []
    for name, spec, n, t in cases:
        ms = {k: [] for k, _ in forms}
        tables = {}
        for _ in range(args.reps):
            for k, f in forms:
                dt, W = timed(f, spec, n, t)
                ms[k].append(round(dt, 3))
                tables[k] = W
        same = all(torch.equal(tables["fused"].view(torch.int32), tables[k].view(torch.int32)) for k in ("ops", "loop"))
        results.append(dict(shape=name, rows=n, trains=t, steps=K_STEPS, loop_ms=ms["loop"], fused_ms=ms["fused"],
                            ops_ms=ms["ops"], train_form=_lib.train_form(spec, True),
                            picked=_lib.mixed_form(spec, True, t),
                            equal=bool(same)))
    print(json.dumps(dict(bench="mixed_run", device=torch.cuda.get_device_name(0), reps=args.reps, results=results)))


if __name__ == "__main__":
    main()
