"""Reference-order soups of runtime shapes on the device: ms per generation.

For WW(3,3), WW(10,3), WW(16,2), Agg(4,4,3), RNN(8,2) and RNN(16,2) at the bench parameters (attack 0.1, learn 0.1,
train 20, respawn) this times one generation of ``SoupEngine(order="sequential")`` -- the
continuation-scheduled generation with the runtime-shape turn (csrc/srnn_generic.hip GOrd) --
eagerly and replayed from hipGraphs, and reports its dependency levels and run form (``--ord-wave
0``: the wide Weightwise shapes' turns on one lane each instead of a group of lanes and the wide
Recurrent shapes' on one lane each instead of a wave, the library knob SRNN_ORD_WAVE).  RNN(16,2) is
in the shape list but not in the default ``--shapes``: its lane steps outlast the step time limit at
100k particles.  Beside it: the
synchronous (Jacobi) soup of the same shape with the wave kernels on and off, and the host serial
loop (``SequentialSoupEngine``) at 2,000 particles scaled per particle.

``ordered-sharded`` times the generation sharded over ranks (csrc/srnn_generic.hip g_soup_ordered_sh)
on the one-rank timing model of 8 ranks (``ExecConfig(ordsh_emulate=8)`` on a one-rank gloo group):
the rank plans every turn, runs 1/8 of the turns of every level and packs, gathers and unpacks their
records.  The model's all-gather never leaves the box -- gloo stages the device records through host
memory -- so inter-GPU transfer time is not in it; the step reports the record bytes of each level
instead.  The rows of the model are invalid by design (a sticky error bit): the step reads the error
word and never calls ``count()``.  The driver runs the step twice, with the wave forms of the level
launches and (``ordered-sharded-lane``) with ``--ord-wave 0``; ``ordered-eager`` of the same run is
the single-rank generation to compare with (profiles/ordered_sharded_runtime_shapes.md).

The driver runs every step in a child process of its own under a time limit and stops at the
first step that fails; each step prints one JSON line.  ``--markdown`` adds the table of
profiles/ordered_runtime_shapes.md.

    python bench/ordered_shapes.py [--n 100000] [--gens 3] [--shapes ww33,ww103,ww162,agg443,rnn82[,rnn162]] [--ord-wave 0|1]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAMS = dict(attacking_rate=0.1, learn_from_rate=0.1, train=20, learn_from_severity=1, remove_divergent=True,
              remove_zero=True, epsilon=1e-4)
SHAPES = {"ww33": ("weightwise", (3, 3)), "ww103": ("weightwise", (10, 3)), "ww162": ("weightwise", (16, 2)),
          "agg443": ("aggregating", (4, 4, 3)),
          "rnn82": ("recurrent", (8, 2)), "rnn162": ("recurrent", (16, 2))}
DEFAULT_SHAPES = tuple(k for k in SHAPES if k != "rnn162")
STEPS = ("ordered-eager", "ordered-graph", "sync-waves", "sync-lanes", "host-serial")
SHARDED_STEPS = ("ordered-sharded", "ordered-sharded-lane")  # (not in the default --steps)
EMULATED_RANKS = 8


def _spec(shape):
    from self_replicating_neural_networks_amd.arch import ArchSpec
    kind, dims = SHAPES[shape]
    return getattr(ArchSpec, kind)(*dims)


def _timed(engine, gens):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    engine.evolve(gens)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / gens * 1e3


def step(name, shape, n, gens, host_n, ord_wave=None):
    import torch
    from self_replicating_neural_networks_amd.config import ExecConfig
    from self_replicating_neural_networks_amd.seq_soup import SequentialSoupEngine
    from self_replicating_neural_networks_amd.soup_engine import SoupEngine

    spec = _spec(shape)
    out = dict(shape=shape, step=name, P=spec.P)
    if name == "host-serial":
        e = SequentialSoupEngine(spec, host_n, PARAMS, seed=1)
        e.evolve(1)
        t = time.perf_counter()
        e.evolve(1)
        ms = (time.perf_counter() - t) * 1e3
        out.update(n=host_n, ms_per_gen=round(ms, 3), us_per_particle=round(ms * 1e3 / host_n, 3),
                   ms_scaled=round(ms * n / host_n, 1), scaled_to=n)
        return out
    if not torch.cuda.is_available():
        raise SystemExit("ordered_shapes: no GPU (a measurement does not fall back to the host)")
    if name in SHARDED_STEPS:
        return sharded_step(out, spec, n, gens, False if name.endswith("-lane") else ord_wave)
    if name.startswith("ordered"):
        ex = ExecConfig(graph_chunks=(2,), ord_wave=ord_wave)
        ex.apply_library()
        e = SoupEngine(spec, n, PARAMS, device="cuda", seed=1, order="sequential", execution=ex)
        assert e._ord_generic, "not a runtime shape"
        if name == "ordered-graph":
            assert e.capture(warmup=1), "graph capture failed"
        e.evolve(2)
        ms = _timed(e, gens)
        lv = e.ordered_levels()
        assert lv["error"] == 0, lv
        out.update(n=n, ms_per_gen=round(ms, 3), levels=lv["levels"], tail=lv["tail"], max_level=lv["max_level"],
                   pending=lv["pending"], run_form=e.ordered_run_form(), stored_attacks=lv["stored_attacks"],
                   scratch_mb=round(e._scratch.numel() / 2 ** 20, 1), census=e.count())
        e.release_graphs()
        return out
    waves = name == "sync-waves"
    ex = ExecConfig(ww_wave=int(waves), rnn_wave=waves, rnn_soup=waves)
    ex.apply_library()
    e = SoupEngine(spec, n, PARAMS, device="cuda", seed=1, execution=ex)
    e.evolve(2)
    ms = _timed(e, gens)
    out.update(n=n, ms_per_gen=round(ms, 3), census=e.count())
    return out


def sharded_step(out, spec, n, gens, ord_wave):
    """The 8-rank timing model of the sharded generation: construct, one untimed generation, `gens`
    timed ones, the error word (never count(): the model's rows are invalid by design)."""
    import socket

    import torch
    import torch.distributed as dist
    from self_replicating_neural_networks_amd.config import ExecConfig
    from self_replicating_neural_networks_amd.ops import _lib
    from self_replicating_neural_networks_amd.parallel.dist import Dist
    from self_replicating_neural_networks_amd.soup_engine import ORD_ERR_EMULATED, SoupEngine

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        ex = ExecConfig(ordsh_emulate=EMULATED_RANKS, ord_wave=ord_wave)
        ex.apply_library()
        e = SoupEngine(spec, n, PARAMS, device="cuda", seed=1, order="sequential", execution=ex,
                       dist=Dist(0, 1, 0, None, force=True))
        assert _lib.is_generic(spec, _lib.OP_SOUP_ORDERED_SH, e.dtype_code), "not a runtime shape"
        e.evolve(1)
        ms = _timed(e, gens)
        err = e.ordered_error()
        assert err == ORD_ERR_EMULATED, f"error word {err}: only the model's own bit may be set"
        lv = e._osrc[:4 * n].view(n, 4)[:, 3]
        own = -(-n // EMULATED_RANKS)
        maxl = int(e._octl[_lib.ORD_MAXLW].item())
        per_level = torch.bincount(lv.clamp(min=0).long(), minlength=maxl + 1)[:maxl + 1].tolist()
        own_level = torch.bincount(lv[:own].clamp(min=0).long(), minlength=maxl + 1)[:maxl + 1].tolist()
        out.update(n=n, ms_per_gen=round(ms, 3), ranks=EMULATED_RANKS, form=e.ordered_sharded_form(),
                   max_level=maxl, turns_per_level=per_level, own_turns_per_level=own_level, record_bytes=e._sh_recb,
                   gathered_mb_per_level=[round(c * e._sh_recb / 2 ** 20, 2) for c in per_level],
                   scratch_mb=round(e._scratch.numel() / 2 ** 20, 1))
    finally:
        dist.destroy_process_group()
    return out


def markdown(rows, n):
    by = {}
    for r in rows:
        by.setdefault(r["shape"], {})[r["step"]] = r
    if any(r["step"] in SHARDED_STEPS for r in rows):
        return sharded_markdown(by)
    lines = [f"| shape | P | ordered eager ms | ordered graph ms | levels (+tail) | sync waves ms | sync lanes ms | "
             f"host loop ms (scaled to {n}) | device vs host |", "|---|---|---|---|---|---|---|---|---|"]
    for shape, d in by.items():
        g = lambda k, f="ms_per_gen": d.get(k, {}).get(f, "not measured")  # noqa: E731
        o = d.get("ordered-graph") or d.get("ordered-eager") or {}
        lv = f"{o.get('levels')} + {o.get('tail')}" if o else "not measured"
        h = d.get("host-serial", {}).get("ms_scaled")
        best = min([x["ms_per_gen"] for k, x in d.items() if k.startswith("ordered")] or [0])
        ratio = f"{h / best:.1f}x" if h and best else "not measured"
        lines.append(f"| {shape} | {o.get('P', '')} | {g('ordered-eager')} | {g('ordered-graph')} | {lv} | "
                     f"{g('sync-waves')} | {g('sync-lanes')} | {h if h else 'not measured'} | {ratio} |")
    return "\n".join(lines)


def sharded_markdown(by):
    lines = ["| shape | P | single rank ms | 8-rank model ms (wave forms) | 8-rank model ms (lane form) | single / model | "
             "levels | turns per level | gathered MiB per level |", "|---|---|---|---|---|---|---|---|---|"]
    for shape, d in by.items():
        g = lambda k, f="ms_per_gen": d.get(k, {}).get(f, "not measured")  # noqa: E731
        w, l = d.get("ordered-sharded", {}), d.get("ordered-sharded-lane", {})
        o = w or l
        ms = [x["ms_per_gen"] for x in (w, l) if x]
        one = d.get("ordered-eager", {}).get("ms_per_gen")
        ratio = f"{one / min(ms):.2f}x" if one and ms else "not measured"
        wave = f"{w['ms_per_gen']} ({w['form']})" if w else "not measured"
        lines.append(f"| {shape} | {o.get('P', '')} | {g('ordered-eager')} | {wave} | {g('ordered-sharded-lane')} | {ratio} | "
                     f"{o.get('max_level', 0) + 1 if o else ''} | {o.get('turns_per_level', '')} | "
                     f"{o.get('gathered_mb_per_level', '')} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--gens", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=2000)
    ap.add_argument("--shapes", default=",".join(DEFAULT_SHAPES))
    ap.add_argument("--steps", default=",".join(STEPS),
                    help="also: ordered-sharded (the driver runs it with the wave forms and, as ordered-sharded-lane, "
                         "with --ord-wave 0)")
    ap.add_argument("--step-timeout", type=int, default=150)
    ap.add_argument("--ord-wave", type=int, choices=(0, 1), default=None,
                    help="reference-order turns of the wide Weightwise shapes on lane groups and of the wide "
                         "Recurrent shapes on waves (1), or on lanes (0); "
                         "default: the library's choice")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("STEP", "SHAPE"))
    args = ap.parse_args()
    if args.child:
        ow = None if args.ord_wave is None else bool(args.ord_wave)
        print(json.dumps(step(args.child[0], args.child[1], args.n, args.gens, args.host_n, ow)), flush=True)
        return 0
    rows = []
    for shape in args.shapes.split(","):
        names = []
        for name in args.steps.split(","):  # (the sharded step: once per form of the level launches)
            names += list(SHARDED_STEPS) if name == "ordered-sharded" else [name]
        for name in names:
            cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--gens", str(args.gens), "--host-n",
                   str(args.host_n), "--child", name, shape]
            if args.ord_wave is not None:
                cmd += ["--ord-wave", str(args.ord_wave)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(shape=shape, step=name, error=f"time limit of {args.step_timeout} s")), flush=True)
                if args.markdown:
                    print(markdown(rows, args.n), flush=True)
                return 124
            if p.returncode != 0:
                err = p.stderr if len(p.stderr) <= 1600 else p.stderr[:800] + " ... " + p.stderr[-800:]
                print(json.dumps(dict(shape=shape, step=name, error=err, rc=p.returncode)), flush=True)
                if args.markdown:
                    print(markdown(rows, args.n), flush=True)
                return p.returncode or 1
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    if args.markdown:
        print(markdown(rows, args.n), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
