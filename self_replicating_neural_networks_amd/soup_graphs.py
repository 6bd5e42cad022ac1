"""hipGraphs of a SoupEngine's generations, as plain functions of the engine: capture (one generation
per ping-pong parity, then multi-generation ``Chunk``s), validation of every graph against eager
generations from a saved state (bitwise, on every rank) before it is kept, replay and release.

What they use of the engine: the schedule (``_generation``, ``_join_side``, ``_prepare_capture``,
``_plan_args``); the host state a generation advances (``_host_state`` / ``_set_host_state``; ``_p``,
``_lists_ready`` and ``time`` by name); the device state (``_state``, compared: COMPARED_STATE, the
census log, the finish ring, the reference-order error words); ``_agree``, ``_ord_side``, ``_sync``,
``_ord_decouple``, ``finish_mode``, ``execution``, ``device``, ``dist``, ``x2``, ``spec``, ``cfg``; and
the graphs they leave on it: ``_graphs``, ``_chunks``, ``_conc``."""
from __future__ import annotations

import sys
from typing import NamedTuple, Optional

import torch

from .ops import _lib


class Chunk(NamedTuple):
    """``gens`` (even) generations from and back to ``parity``; ``side``: a two-graph chunk's plans."""
    graph: torch.cuda.CUDAGraph
    parity: int
    gens: int
    side: Optional[torch.cuda.CUDAGraph]


def chunk_sizes(eng):
    """Generations per multi-generation graph (ExecConfig.graph_chunks, even sizes): an evolve of K
    generations replays the largest that fit, so a short timed region pays few launches and few
    finish launches (one 20-generation graph for K = 20, 20 + 20 + 8 + 2 for K = 50)."""
    return sorted({int(x) for x in eng.execution.graph_chunks}, reverse=True)


def _capture(eng, failed: str, *parts):
    """Capture each ``(stream, body)`` of ``parts`` in a graph of its own, in turn, and put the host
    state back (the bodies advance it as if they had run, a failed one part of it).  The graphs, or
    None when any rank's capture failed (``failed`` on stderr): every rank agrees, so a rank whose
    capture failed never leaves the others waiting inside a collective."""
    st = eng._host_state()
    graphs = []
    try:
        for stream, body in parts:
            g = torch.cuda.CUDAGraph()
            # thread_local: the process group's watchdog thread keeps querying events
            with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
                body()
            graphs.append(g)
    except Exception as e:  # noqa: BLE001 -- any capture failure -> the caller's fallback
        print(failed.format(f"{type(e).__name__}: {e}"), file=sys.stderr)
        graphs = None
    eng._set_host_state(st)
    return graphs if eng._agree(graphs is not None) else None


def capture(eng, warmup: int = 1, validate: bool = True) -> bool:
    """Capture the generation for both ping-pong parities in two hipGraphs (ROCm device).
    Everything that changes per generation lives in device memory (generation counter, next uid),
    so replays advance the soup exactly like the eager path.  Sharded engines capture their RCCL
    collective inside the graph (one all-to-all per generation on the comm stream, joined back);
    ``validate`` then replays generations from a saved state, compares them bitwise with the eager
    path on every rank and keeps the graphs only if all ranks agree."""
    if eng.device.type != "cuda" or (eng.dist.world > 1 and not eng.execution.sharded_graph):
        return False
    if eng.dist.enabled and (not eng.x2 or eng.dist.native is None):
        # (torch's process-group collectives are not captured: their watchdog thread queries events
        # recorded by the capturing stream)
        return False

    def generation():
        eng._generation()  # flips _p during capture (nothing ran)
        eng._join_side()

    s = torch.cuda.Stream(eng.device)
    s.wait_stream(torch.cuda.current_stream(eng.device))
    # max(warmup, 1) eager generations in all: the last one runs between the capture of the
    # multi-generation graphs of the two parities (below)
    with torch.cuda.stream(s):
        for _ in range(max(warmup, 1) - 1):
            eng.time += 1
            eng._generation()
        eng._join_side()
        eng._prepare_capture()
    torch.cuda.current_stream(eng.device).wait_stream(s)
    torch.cuda.synchronize(eng.device)
    graphs = _capture(eng, "soup graph capture failed ({}); running eagerly", (s, generation), (s, generation))
    if graphs is not None and validate:
        if not eng._agree(_validate_replay(eng, lambda: [g.replay() for g in graphs], 2)):
            graphs = None
    eng._graphs = graphs[::-1] if graphs is not None and eng._p == 1 else graphs  # (by parity)
    if graphs is None:
        eng.time += 1  # the last warmup generation, eagerly
        generation()
        return False
    eng._chunks = []
    _capture_chunks(eng, s)
    # the last warmup generation (eager), then the same chunks from the other parity: an
    # evolve replays multi-generation graphs whatever parity it starts at (an odd
    # warmup would otherwise leave every later generation on single-generation graphs)
    with torch.cuda.stream(s):
        eng.time += 1
        generation()
    torch.cuda.current_stream(eng.device).wait_stream(s)
    torch.cuda.synchronize(eng.device)
    if eng._chunks:
        _capture_chunks(eng, s)
    return True


def _capture_chunks(eng, s):
    """Multi-generation graphs from (and back to) the current parity, added to _chunks (largest first)."""
    for G in chunk_sizes(eng):
        ch = _capture_chunk(eng, s, G)
        if ch is None:
            break
        eng._chunks.append(ch)
    eng._chunks.sort(key=lambda c: -c.gens)


def _capture_chunk(eng, s, G) -> Optional[Chunk]:
    """A graph of G consecutive generations (G even: it starts and ends at the current parity)
    replayed as one launch, removing the per-generation graph-launch gap; validated bitwise against
    G eager generations (all ranks agree or none use it).  Reference order with the side-stream plan
    (ExecConfig.ord_graph_sync): first as TWO graphs -- main: G x (run + close, the close waiting for
    the next plan) + the batched finish; side stream: G x (gate on the run counter, plan of the next
    generation, done count) -- ordered by device counters (SRNN_F_ORD_SYNC) instead of a cross-queue
    join per generation (~10 us of idle queue each, profiles/r6a); one graph if that fails."""
    p0 = eng._p

    def generations():
        for _ in range(G):
            eng._generation()
        eng._join_side()

    def plans():
        for g in range(G):
            eng._p = p0 ^ (g & 1)
            _lib.run(_lib.OP_ORD_PLAN, eng.spec, eng._plan_args(True), eng.cfg)

    if eng._ord_decouple and eng._lists_ready and _streams_concurrent(eng):
        eng._sync = True
        try:
            graphs = _capture(eng, "two-graph capture failed ({}); one graph", (s, generations), (eng._ord_side, plans))
        finally:
            eng._sync = False
        if graphs is not None:
            ch = Chunk(graphs[0], p0, G, graphs[1])
            if eng._agree(_validate_replay(eng, lambda: replay_chunk(eng, ch), G, chunk=True,
                                           ring=eng.finish_mode == "batch")):
                return ch
    graphs = _capture(eng, "multi-generation graph capture failed ({})", (s, generations))
    if graphs is not None and eng._agree(_validate_replay(eng, graphs[0].replay, G, chunk=True)):
        return Chunk(graphs[0], p0, G, None)
    return None


def _streams_concurrent(eng) -> bool:
    """(once per engine) whether kernels on the side stream and the current one run at the same
    time -- a two-graph chunk's counters need it: under a profiler that serialises kernels
    (rocprofv3 --pmc) or on a shared hardware queue every wait would run into its timeout.
    Agreed over the ranks."""
    if eng._conc is None:
        ok = _lib.streams_concurrent(eng._ord_side, torch.cuda.current_stream(eng.device), eng.device)
        if not ok:
            print("side stream does not run beside the current one (serialising profiler?): "
                  "one-graph chunks", file=sys.stderr)
        eng._conc = eng._agree(ok)
    return eng._conc


def replay_chunk(eng, ch: Chunk):
    """Replay a multi-generation chunk; a two-graph chunk's side graph first, on the side stream
    (after the work already queued on this one: its first plan overwrites the set of the
    generation before the chunk), the two then run on their own, ordered by the counters."""
    if ch.side is not None:
        eng._ord_side.wait_stream(torch.cuda.current_stream(eng.device))
        with torch.cuda.stream(eng._ord_side):
            ch.side.replay()
    ch.graph.replay()


def release(eng):
    """Drop the captured graphs (before tearing down the process group: an RCCL
    communicator must not be destroyed while graph executables still reference it)."""
    if eng._graphs is not None or eng._chunks:
        torch.cuda.synchronize(eng.device)
        for g in (eng._graphs or []) + [c.graph for c in eng._chunks] + [c.side for c in eng._chunks if c.side]:
            g.reset()
        eng._graphs, eng._chunks = None, []


def _validate_replay(eng, replay, gens: int, chunk: bool = False, ring: bool = False) -> bool:
    """Run ``gens`` eager generations from the current state, restore it, run ``replay`` (the captured
    equivalent), compare bitwise, restore again.  ``chunk`` / ``ring``: the census log / the finish
    ring compared too."""
    def synchronize():
        if eng.device.type == "cuda":
            torch.cuda.synchronize(eng.device)

    def restore():
        for t, v in zip(state, saved):
            t.copy_(v)
        eng._set_host_state(host0)

    state = eng._state()
    saved = [t.clone() for t in state]
    host0 = eng._host_state()
    for _ in range(gens):
        eng._generation()
    eng._join_side()
    synchronize()
    host1 = eng._host_state()
    eager = [t.clone() for t in state]
    restore()
    replay()
    eng._set_host_state(host1)  # (what a replay leaves behind is the eager generations' host state)
    synchronize()
    keep = {id(t) for t in eng._state(eng.COMPARED_STATE)}
    if chunk and eng._census_log is not None:
        # (a chunk finishes its generations in the launches the eager generations use, so the census
        # log rows agree; two single-generation graphs finish one by one, the eager pair at once)
        keep.add(id(eng._census_log))
    if ring and eng._bs_ring is not None:
        # (a chunk batches its finishes like the eager generations: every generation's census and
        # ballots, wherever they ran, compared too)
        keep.add(id(eng._bs_ring))
    same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8))
               for x, y in zip(state, eager) if id(x) in keep)
    # (reference order: and no error bit the eager generations did not raise either)
    for x, y in zip(state, eager):
        if x is eng._octl or x is eng._octl1:
            same = same and int(x[_lib.ORD_ERRW]) == int(y[_lib.ORD_ERRW])
    restore()
    synchronize()
    return same
