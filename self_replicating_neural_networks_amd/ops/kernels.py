"""Population operators on torch tensors, executed by libsrnn.so.

Every function takes a weight table ``W`` of shape ``[N, spec.PP]`` (float32, contiguous)
on either the CPU (host thread-pool path of the native library) or a ROCm device (HIP
kernels for gfx950, lane-per-particle).  Both paths run the *same* C++ per-particle code
(csrc/srnn_kernels.h); the numpy oracle in ``..oracle`` is the independent reference.

Shapes are checked on the host before anything is launched.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import SrnnArgs

_CHECKED = os.environ.get("SRNN_CHECKED", "0") == "1"


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# weight-table storage formats; arithmetic is fp32 in registers for all of them
TABLE_DTYPES = {torch.float32: _lib.DTYPE_FP32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_FP16}


def dtype_code(dtype: torch.dtype) -> int:
    if dtype not in TABLE_DTYPES:
        raise TypeError(f"weight tables must be float32, bfloat16 or float16, got {dtype}")
    return TABLE_DTYPES[dtype]


def _check_table(spec, W: torch.Tensor, name="W", like: Optional[torch.Tensor] = None) -> int:
    code = dtype_code(W.dtype)
    if like is not None and W.dtype != like.dtype:
        raise TypeError(f"{name} has dtype {W.dtype}, expected {like.dtype} (same storage as W)")
    if W.dim() != 2 or W.shape[1] != spec.PP:
        raise ValueError(f"{name} must have shape [N, {spec.PP}] for {spec}, got {tuple(W.shape)}")
    if not W.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return code


def _check_idx(idx: Optional[torch.Tensor], n_items: int, n_rows: int, dev, name: str):
    if idx is None:
        if n_items > n_rows:
            raise ValueError(f"{name}: {n_items} items but only {n_rows} rows")
        return
    if idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() != n_items or not idx.is_contiguous():
        raise ValueError(f"{name} must be a contiguous int64 vector of length {n_items}")
    if idx.device != dev:
        raise ValueError(f"{name} is on {idx.device}, expected {dev}")
    if n_items and (idx.device.type == "cpu" or _CHECKED):
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= n_rows:
            raise IndexError(f"{name} out of range [0, {n_rows}): min {lo} max {hi}")


def is_wave_per_particle(spec, W: Optional[torch.Tensor] = None) -> bool:
    """Nets too large for the register kernels run wave-per-particle: aggregating nets
    (csrc/srnn_bignet.hip, chunk-state multi-step) and width >= 16 weightwise nets
    (csrc/srnn_wide.hip, MFMA) -- for the shapes those files instantiate; every other
    shape runs on the runtime-shape engine (csrc/srnn_generic.hip).  ``W``: the table the
    question is about (host tables and, for run_fixpoint, 16-bit or shuffled ones run on
    the runtime-shape engine); default: a float32 device table."""
    if W is not None and W.device.type != "cuda":
        return False
    dt = dtype_code(W.dtype) if W is not None else _lib.DTYPE_FP32
    return (((spec.kind == "aggregating" and spec.P > 64) or (spec.kind == "weightwise" and spec.width >= 16))
            and not _lib.is_generic(spec, _lib.OP_RUN_FIXPOINT, dt))


def needs_chunk_state_temp(spec, W: Optional[torch.Tensor] = None) -> bool:
    """True when run_fixpoint of this table runs on the chunk-state kernels of the big
    aggregating nets (k_big_fix1/2/3), which need the caller's ``temp``."""
    return spec.kind == "aggregating" and spec.P > 64 and is_wave_per_particle(spec, W)


def _chunk_columns(spec, device) -> torch.Tensor:
    """Chunk index of every weight (``ArchSpec.chunks``), int64[P]."""
    idx = torch.empty(spec.P, dtype=torch.int64)
    for c, (start, length) in enumerate(spec.chunks):
        idx[start:start + length] = c
    return idx.to(device)


@dataclasses.dataclass
class StateTrajectory:
    """Compact self-application trajectory of an unshuffled aggregating net: after its first
    self-application the row is constant over each aggregation chunk, so step ``s >= 1`` of
    particle ``p`` is the ``A`` chunk values ``states[s - 1, p]`` (zero past ``nsteps[p]``)
    and ``row0`` holds the input rows."""
    spec: object
    row0: torch.Tensor     # [N, PP], the table's dtype
    states: torch.Tensor   # [steps, N, A] float32
    nsteps: torch.Tensor   # [N] int32

    @property
    def steps(self) -> int:
        return self.states.shape[0]

    def _expand(self, st: torch.Tensor, first_step: int) -> torch.Tensor:
        """[k, N, A] states of steps first_step .. first_step + k - 1 -> rows [k, N, PP]."""
        k, n = st.shape[0], st.shape[1]
        out = torch.zeros((k, n, self.spec.PP), dtype=self.row0.dtype, device=st.device)
        out[:, :, :self.spec.P] = st[:, :, _chunk_columns(self.spec, st.device)].to(self.row0.dtype)
        step = torch.arange(first_step, first_step + k, device=st.device)[:, None]
        out[step > self.nsteps.to(st.device)[None, :].to(torch.int64)] = 0
        return out

    def rows(self, s: int) -> torch.Tensor:
        """The rows [N, PP] after step ``s`` (0: the input); zero rows past ``nsteps``."""
        if not 0 <= s <= self.steps:
            raise IndexError(f"step {s} outside the recording [0, {self.steps}]")
        return self.row0.clone() if s == 0 else self._expand(self.states[s - 1:s], s)[0]

    def full(self) -> torch.Tensor:
        """The dense trajectory [(steps+1), N, PP], what ``record=True`` returns."""
        return torch.cat([self.row0[None], self._expand(self.states, 1)])

    def particle(self, r: int):
        """Particle ``r``'s recorded steps, numpy [nsteps[r]+1, P]."""
        k = int(self.nsteps[r])
        rows = self.states[:k, r][:, _chunk_columns(self.spec, self.states.device)].to(self.row0.dtype)
        return torch.cat([self.row0[r:r + 1, :self.spec.P], rows]).float().cpu().numpy()


def _base_args(W: torch.Tensor, seed: int = 0, ctr: int = 0, scratch: Optional[torch.Tensor] = None) -> SrnnArgs:
    """``scratch``: device bytes for the runtime-shape engine (csrc/srnn_generic.hip); when
    omitted the library uses its own cached buffer (not allowed inside a graph capture)."""
    a = SrnnArgs()
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.ctr = int(ctr) & 0xFFFFFFFF
    if W.device.type == "cuda":
        a.dev = 1
        a.stream = ctypes.c_void_p(torch.cuda.current_stream(W.device).cuda_stream)
        if scratch is not None:
            a.scratch, a.scratch_bytes = _p(scratch), scratch.numel() * scratch.element_size()
    else:
        a.dev = 0
    return a


def _uid(uid: Optional[torch.Tensor], n: int, dev):
    if uid is None:
        return None
    if uid.dtype != torch.int64 or uid.numel() < n or uid.device != dev or not uid.is_contiguous():
        raise ValueError("uid must be a contiguous int64 tensor on the table's device covering every row")
    return uid


def init_rows(spec, W: torch.Tensor, uid: torch.Tensor, seed: int) -> torch.Tensor:
    """W[i] = fresh particle (glorot kernels, orthogonal recurrent kernels) keyed by uid[i]."""
    dt = _check_table(spec, W)
    n = W.shape[0]
    a = _base_args(W, seed)
    a.n = n
    a.W = _p(W)
    a.uid = _p(_uid(uid, n, W.device))
    _lib.run(_lib.OP_INIT, spec, a, dtype=dt)
    return W


def apply(spec, W: torch.Tensor, out: torch.Tensor, idx_f=None, idx_t=None, idx_o=None, n=None,
          uid=None, seed=0, ctr=0) -> torch.Tensor:
    """out[idx_o[i]] = f_{W[idx_f[i]]}(W[idx_t[i]])  (attack; reference code/network.py:112-118)."""
    dt = _check_table(spec, W)
    _check_table(spec, out, "out", like=W)
    if n is None:
        n = (idx_t if idx_t is not None else idx_f if idx_f is not None else W).shape[0]
    for nm, ix, rows in (("idx_f", idx_f, W.shape[0]), ("idx_t", idx_t, W.shape[0]), ("idx_o", idx_o, out.shape[0])):
        _check_idx(ix, n, rows, W.device, nm)
    a = _base_args(W, seed, ctr)
    a.n = n
    a.W, a.W2 = _p(W), _p(out)
    a.idx_f, a.idx_t, a.idx_o = _p(idx_f), _p(idx_t), _p(idx_o)
    a.uid = _p(_uid(uid, W.shape[0], W.device))
    _lib.run(_lib.OP_APPLY, spec, a, dtype=dt)
    return out


def run_fixpoint(spec, W: torch.Tensor, steps: int, eps: float, early_exit: bool = True, with_sec: bool = True,
                 record=False, uid=None, seed=0, ctr=0):
    """Per-row ``FixpointExperiment.run_net`` (code/experiment.py:70-91), in place.

    Returns (class int8[N], steps int32[N], trajectory).  ``record=True``: the dense trajectory
    [(steps+1), N, PP] (row 0 the input, zero rows past a particle's last step), for every net and
    table; ``record="state"``: a ``StateTrajectory`` (unshuffled aggregating nets only, ValueError
    otherwise); ``record=False``: None."""
    dt = _check_table(spec, W)
    if record is not False and record is not True and record != "state":
        raise ValueError(f"record must be False, True or 'state', got {record!r}")
    compact = record == "state"
    if compact and not (spec.kind == "aggregating" and spec.shuffler == "none"):
        raise ValueError(f"record='state' needs an unshuffled aggregating net (chunk-constant rows), got {spec}")
    n, steps = W.shape[0], int(steps)
    cls = torch.empty(n, dtype=torch.int8, device=W.device)
    nsteps = torch.empty(n, dtype=torch.int32, device=W.device)
    a = _base_args(W, seed, ctr)
    a.n, a.steps, a.eps, a.early_exit = n, steps, float(eps), int(bool(early_exit))
    a.flags = _lib.FLAG_FIX_SEC if with_sec else 0
    a.W, a.cls, a.nsteps = _p(W), _p(cls), _p(nsteps)
    a.uid = _p(_uid(uid, n, W.device))
    # the route of THIS table (device, storage format, shuffler): the chunk-state kernels serve
    # float32 device tables of unshuffled big aggregating nets, the runtime-shape engine the rest
    chunk_state = needs_chunk_state_temp(spec, W)
    traj = states = row0 = temp = None
    if compact and chunk_state:  # the kernels write the chunk states themselves
        row0 = W.clone()
        states = torch.zeros((max(steps, 0), n, spec.aggregates), dtype=torch.float32, device=W.device)
        a.traj = _p(states)
        a.flags |= _lib.FLAG_TRAJ_STATE
    elif record:
        traj = torch.zeros((max(steps, 0) + 1, n, spec.PP), dtype=W.dtype, device=W.device)
        a.traj = _p(traj)
    if chunk_state:
        temp = torch.empty(_lib.big_fix_temp_bytes(spec, n, steps, dense=traj is not None), dtype=torch.uint8,
                           device=W.device)
        a.temp, a.temp_bytes = _p(temp), temp.numel()
    _lib.run(_lib.OP_RUN_FIXPOINT, spec, a, dtype=dt)
    if compact:
        if states is None:  # recorded densely: one weight per chunk
            starts = torch.tensor([c[0] for c in spec.chunks], dtype=torch.int64, device=W.device)
            row0, states = traj[0].clone(), traj[1:, :, starts].float()
        return cls, nsteps, StateTrajectory(spec, row0, states, nsteps)
    return cls, nsteps, traj


def vary_run(spec, W: torch.Tensor, steps: int, eps: float, uid=None, seed=0, ctr=0):
    """Known-fixpoint-variation dynamics (code/setups/known-fixpoint-variation.py:66-83).
    Returns (time_to_vergence int32[N], time_as_fixpoint float32[N])."""
    dt = _check_table(spec, W)
    n = W.shape[0]
    tts = torch.empty(n, dtype=torch.int32, device=W.device)
    taf = torch.empty(n, dtype=torch.float32, device=W.device)
    a = _base_args(W, seed, ctr)
    a.n, a.steps, a.eps = n, int(steps), float(eps)
    a.W, a.nsteps, a.loss = _p(W), _p(tts), _p(taf)
    a.uid = _p(_uid(uid, n, W.device))
    _lib.run(_lib.OP_VARY_RUN, spec, a, dtype=dt)
    return tts, taf


def perturb(spec, W: torch.Tensor, e: float, uid=None, seed=0, ctr=0) -> torch.Tensor:
    """w +-= U(0,1)*e with p=1/2 per weight (reference ``vary``, known-fixpoint-variation.py:37-46)."""
    dt = _check_table(spec, W)
    a = _base_args(W, seed, ctr)
    a.n, a.eps = W.shape[0], float(e)
    a.W = _p(W)
    a.uid = _p(_uid(uid, W.shape[0], W.device))
    _lib.run(_lib.OP_PERTURB, spec, a, dtype=dt)
    return W


def train(spec, W: torch.Tensor, epochs: int = 1, lr: float = 0.01, shuffle: bool = True, uid=None, seed=0,
          ctr=0, rows: Optional[int] = None) -> torch.Tensor:
    """``epochs`` self-train epochs per row, in place (code/network.py:613-618). Returns last loss [N]."""
    dt = _check_table(spec, W)
    n = W.shape[0] if rows is None else rows
    loss = torch.empty(n, dtype=torch.float32, device=W.device)
    a = _base_args(W, seed, ctr)
    a.n, a.epochs, a.lr = n, int(epochs), float(lr)
    a.flags = _lib.FLAG_SHUFFLE if shuffle else 0
    a.W, a.loss = _p(W), _p(loss)
    a.uid = _p(_uid(uid, n, W.device))
    _lib.run(_lib.OP_TRAIN, spec, a, dtype=dt)
    return loss


def learn_from(spec, W: torch.Tensor, teachers: torch.Tensor, idx_t=None, epochs: int = 1, lr: float = 0.01,
               shuffle: bool = True, uid=None, seed=0, ctr=0) -> torch.Tensor:
    """Row i trains ``epochs`` epochs on the samples of teachers[idx_t[i]] (code/network.py:620-626)."""
    dt = _check_table(spec, W)
    _check_table(spec, teachers, "teachers", like=W)
    n = W.shape[0]
    _check_idx(idx_t, n, teachers.shape[0], W.device, "idx_t")
    loss = torch.empty(n, dtype=torch.float32, device=W.device)
    a = _base_args(W, seed, ctr)
    a.n, a.epochs, a.lr = n, int(epochs), float(lr)
    a.flags = _lib.FLAG_SHUFFLE if shuffle else 0
    a.W, a.W2, a.idx_t, a.loss = _p(W), _p(teachers), _p(idx_t), _p(loss)
    a.uid = _p(_uid(uid, n, W.device))
    _lib.run(_lib.OP_LEARN, spec, a, dtype=dt)
    return loss


def classify(spec, W: torch.Tensor, eps: float, with_sec: bool = True, uid=None, seed=0, ctr=0,
             counts: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, key_offset: int = 0):
    """Per-row class (0 divergent, 1 fix_zero, 2 fix_other, 3 fix_sec, 4 other) and the
    5-bin histogram (reference code/experiment.py:79-91, code/soup.py:89-103)."""
    dt = _check_table(spec, W)
    n = W.shape[0]
    cls = torch.empty(n, dtype=torch.int8, device=W.device)
    if counts is None:
        counts = torch.zeros(5, dtype=torch.int64, device=W.device)
    a = _base_args(W, seed, ctr, scratch)
    a.n, a.eps = n, float(eps)
    a.lo = int(key_offset)  # without uids, row i's random streams are keyed by key_offset + i
    a.flags = _lib.FLAG_FIX_SEC if with_sec else 0
    a.W, a.cls, a.counts = _p(W), _p(cls), _p(counts)
    a.uid = _p(_uid(uid, n, W.device))
    _lib.run(_lib.OP_CLASSIFY, spec, a, dtype=dt)
    return cls, counts


# -------------------------------------------------------------------------------- mixed runs
# One self-attack followed by ``trains`` self-train epochs per step, until a net is divergent or a
# fixpoint (reference code/experiment.py:94-109, code/setups/mixed-self-fixpoints.py:81-86).
# Counter schedule (docs/semantics.md): step s applies at c = ctr + s * (trains + 2), trains at
# c + 1 .. c + trains; the final classification is at ctr + steps * (trains + 2).
def _mixed_outputs(spec, W, steps, record):
    n = W.shape[0]
    nsteps = torch.zeros(n, dtype=torch.int32, device=W.device)
    loss = torch.zeros(n, dtype=torch.float32, device=W.device)
    traj = torch.zeros((max(steps, 0) + 1, n, spec.PP), dtype=W.dtype, device=W.device) if record else None
    return nsteps, loss, traj


def _check_mixed(trains, steps):
    trains, steps = int(trains), int(steps)
    if trains < 0 or steps < 0:
        raise ValueError(f"mixed run: trains and steps must be >= 0, got trains={trains} steps={steps}")
    return trains, steps


def run_mixed_fused(spec, W: torch.Tensor, trains: int, steps: int, eps: float, check_first: bool = True,
                    with_sec: bool = True, lr: float = 0.01, shuffle: bool = True, record: bool = False, uid=None,
                    seed=0, ctr=0):
    """The mixed run as one ``OP_RUN_MIXED`` launch (a lane per particle, the weights in registers or
    lane scratch across every self-attack and its epochs), in place.  See ``run_mixed``."""
    dt = _check_table(spec, W)
    trains, steps = _check_mixed(trains, steps)
    n = W.shape[0]
    cls = torch.empty(n, dtype=torch.int8, device=W.device)
    nsteps, loss, traj = _mixed_outputs(spec, W, steps, record)
    a = _base_args(W, seed, ctr)
    a.n, a.steps, a.epochs, a.eps, a.lr = n, steps, trains, float(eps), float(lr)
    a.early_exit = 1 if check_first else 2
    a.flags = (_lib.FLAG_FIX_SEC if with_sec else 0) | (_lib.FLAG_SHUFFLE if shuffle else 0)
    a.W, a.cls, a.nsteps, a.loss, a.traj = _p(W), _p(cls), _p(nsteps), _p(loss), _p(traj)
    a.uid = _p(_uid(uid, n, W.device))
    _lib.run(_lib.OP_RUN_MIXED, spec, a, dtype=dt)
    return cls, nsteps, loss, traj


def run_mixed_ops(spec, W: torch.Tensor, trains: int, steps: int, eps: float, check_first: bool = True,
                  with_sec: bool = True, lr: float = 0.01, shuffle: bool = True, record: bool = False, uid=None,
                  seed=0, ctr=0):
    """The mixed run built from the existing operators on the same counter schedule: per step
    ``classify(with_sec=False)`` and ``run_fixpoint(steps=1, early_exit=False)`` at ``c``, ``train(trains)``
    at ``c + 1``; the final ``classify`` at ``ctr + steps * (trains + 2)``.  The rows still running are
    gathered (with their uids, which key every random stream) into a compact table before each step
    and scattered back after it, so stopped rows cost nothing.  Bitwise equal to ``run_mixed_fused``;
    the form that keeps the wave / row training kernels of the shapes that have them."""
    _check_table(spec, W)
    trains, steps = _check_mixed(trains, steps)
    n = W.shape[0]
    nsteps, loss, traj = _mixed_outputs(spec, W, steps, record)
    keys = _uid(uid, n, W.device)
    if keys is None:  # without a uid column a row's streams are keyed by its index
        keys = torch.arange(n, dtype=torch.int64, device=W.device)
    if traj is not None:
        traj[0] = W
    idx = torch.arange(n, dtype=torch.int64, device=W.device)
    for s in range(steps):
        if idx.numel() == 0:
            break
        c = ctr + s * (trains + 2)
        sub, su = W[idx].contiguous(), keys[idx].contiguous()
        if s > 0 or check_first:
            k, _ = classify(spec, sub, eps, with_sec=False, uid=su, seed=seed, ctr=c)
            go = k == 4  # neither divergent nor a fixpoint
            idx = idx[go]
            if idx.numel() == 0:
                break
            sub, su = sub[go].contiguous(), su[go].contiguous()
        run_fixpoint(spec, sub, 1, eps, early_exit=False, with_sec=False, uid=su, seed=seed, ctr=c)
        if trains:
            loss[idx] = train(spec, sub, trains, lr, shuffle, uid=su, seed=seed, ctr=c + 1)
        W[idx] = sub
        nsteps[idx] += 1
        if traj is not None:
            traj[s + 1, idx] = sub
    cls, _ = classify(spec, W, eps, with_sec, uid=keys, seed=seed, ctr=ctr + steps * (trains + 2))
    return cls, nsteps, loss, traj


def run_mixed(spec, W: torch.Tensor, trains: int, steps: int, eps: float, check_first: bool = True,
              with_sec: bool = True, lr: float = 0.01, shuffle: bool = True, record: bool = False, uid=None,
              seed=0, ctr=0):
    """Per-row ``MixedFixpointExperiment.run_net`` (code/experiment.py:94-109), in place: up to ``steps``
    times one self-attack and ``trains`` self-train epochs, a row stopping once it is divergent or a
    fixpoint.  ``check_first=False`` leaves step 0 unchecked (code/setups/mixed-self-fixpoints.py:81-86).

    Returns (class int8[N], steps int32[N], last epoch's loss float32[N] -- 0 where no epoch ran,
    trajectory [(steps+1), N, PP] with ``record`` -- row 0 the input, zero rows past a particle's last
    step -- else None).

    The form follows the shape (``_lib.mixed_form``): where ``OP_TRAIN`` runs a lane per particle
    (``_lib.train_form``) the whole run is one fused launch; where it has a wave or row kernel the op
    sequence keeps that kernel.  On the device the lane shapes also take the op sequence from a
    measured number of epochs per step on (long training on the few rows still running: only the op
    sequence compacts them).  Both forms give the same bits."""
    form = _lib.mixed_form(spec, W.device.type == "cuda", _check_mixed(trains, steps)[0], dtype_code(W.dtype))
    f = run_mixed_ops if form == "ops" else run_mixed_fused
    return f(spec, W, trains, steps, eps, check_first, with_sec, lr, shuffle, record, uid, seed, ctr)
