"""Float32 numpy oracle of the engine's EXACT arithmetic (Weightwise, Aggregating, Recurrent).

``oracle.core`` states the reference semantics with numpy's own
rounding: every product rounded, then added.  The native code (csrc/srnn_core.h), built
with ``-ffp-contract=on`` for the device and ``-Xarch_host -mfma`` for the host, FUSES the
multiply-adds its source writes as ``fmaf`` or as one ``a*b + c`` expression -- one
rounding instead of two -- in a fixed order.  Chaotic particle dynamics amplify that 1-ulp
difference, so ``core`` can pin the engine only loosely over many SGD steps.

This module replays the engine's operation sequence step for step:

* ``dense_fwd``         acc = x0*k0, then acc = fma(x_i, k_i, acc)       (csrc dense_fwd)
* folded SGD step       so = -(2 lr) * err; si = K . so (pre-update K, the same chain);
                        K[i, j] = fma(x_i, so_j, K[i, j])                (MLP::backward_update)
* epoch loss            acc = fma(err, err, acc); loss = acc / P        (train_epochs)
* glorot init           w = fma(2 lim, u, -lim)                          (glorot_fill)

Aggregating and Recurrent nets follow the same rule (``-ffp-contract=on``: ``a*b + c`` fuses
inside one expression, never across statements); their steps, transcribed from csrc:

* ``aggregate``         mean: sequential double sum, divided in double, one cast; max /
                        max_ref: the ``v > m`` scan from the chunk's first weight
* Aggregating epoch     e = h - g; loss = fma(e, e, loss); gy = (2 e) / A; so = (-lr) * gy,
                        then the folded step above; loss / A           (Aggregating::train_epoch)
* Recurrent cell        hn = x.K + hp.R: two dense_fwd chains, one plain add (Recurrent::cell)
* Recurrent BPTT        dh = dtop + carry; gw = fma(x_i, dh_j, gw); dx and the new carry are
                        chains fma(w_ij, dh_j, acc) from acc = 0; w = fma(gw, -lr, w) at the
                        epoch's end                                     (cell_bwd, train_epoch)

The Recurrent orthogonal init goes through libm and has no exact transcription: Recurrent
rows start from the engine's own init.  FFT nets are not covered.

A fused multiply-add of float32 operands is computed exactly: the product is exact in
float64 (48 significant bits), the sum is rounded to ODD at 53 bits (TwoSum gives the
rounding error; an inexact sum with an even last bit moves one ulp toward the error), then
to float32.  53 >= 24 + 2, so the final rounding equals that of the infinitely precise
``a*b + c`` -- ``tests/test_exact_oracle.py`` checks it against rational arithmetic.  The
oracle equals the host and device engines bitwise: the tests check it at zero tolerance on
the host and on the device, and ``smoke()`` checks a device generation against it.

The reference's sequential soup (code/soup.py:51-87) is ``seq_generation``; the native
serial loop is csrc Item::soup_seq_one and the level-scheduled GPU generation
csrc/srnn_ordered.h, both bitwise equal to it.
"""
from __future__ import annotations

import numpy as np

from ..arch import ArchSpec
from . import core as C

F32 = np.float32
F64 = np.float64


_U64 = np.uint64
_LOW29, _TIE, _ABS, _SUBN = _U64((1 << 29) - 1), _U64(1 << 28), _U64((1 << 63) - 1), _U64((1023 - 126) << 52)


def _f32(x):
    return x if type(x) is np.ndarray and x.dtype == F32 else np.asarray(x, F32)


def fma(a, b, c):
    """float32 fma(a, b, c), correctly rounded (see the module docstring).

    The float64 sum s = RN53(a*b + c) rounds to the same float32 as the exact value unless s
    lies exactly on a midpoint of the float32 grid (rounding to float64 is monotone and the
    midpoints are float64 numbers, so it cannot cross one, only land on it).  In the normal
    range and at the overflow threshold those are the s whose low 29 bits are 1 0...0; below
    2^-126 the grid is coarser, so every such s counts.  Only then is the sum redone rounded to
    odd: TwoSum gives its error, and an inexact s with an even last bit moves one ulp toward it."""
    a, b, c = _f32(a), _f32(b), _f32(c)
    p = np.multiply(a, b, dtype=F64)  # exact: 24 + 24 bits
    s = np.asarray(np.add(p, c, dtype=F64))
    u = s.view(_U64)
    tiny = np.count_nonzero((u & _ABS) < _SUBN)  # (exact zeros included: they need no second look)
    if np.count_nonzero((u & _LOW29) == _TIE) or (tiny and tiny != s.size - np.count_nonzero(s)):
        bb = s - p
        err = (p - (s - bb)) + np.subtract(c, bb, dtype=F64)  # p + c == s + err exactly (NaN: s not finite)
        fix = (err != 0) & np.isfinite(err) & ((u & _U64(1)) == 0)
        if fix.any():
            s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _check(spec: ArchSpec, init=False):
    if spec.kind == "fft" or (init and spec.kind == "recurrent"):
        raise NotImplementedError("the exact oracle covers Weightwise, Aggregating and Recurrent nets"
                                  " (no exact init of Recurrent nets: the orthogonal kernels go through libm)")


# ------------------------------------------------------------------------------ init
def init(spec: ArchSpec, uids, seed) -> np.ndarray:
    """glorot_fill with the device's fused ``-lim + (2 lim) * u`` (Weightwise and Aggregating nets)."""
    _check(spec, init=True)
    uids = np.asarray(uids, dtype=np.uint64).reshape(-1)
    w = np.zeros((uids.shape[0], spec.P), dtype=F32)
    for (r, c), off in zip(spec.layer_shapes, spec.offsets):
        lim = F32(np.sqrt(F32(6.0) / F32(r + c)))
        n = r * c
        for b in range((n + 3) // 4):
            words = C.draw(seed, uids, off * 1024 + b, C.P_INIT)
            for q in range(4):
                k = b * 4 + q
                if k < n:
                    w[:, off + k] = fma(F32(2.0) * lim, C.u01(words[q]), -lim)
    return w


# ------------------------------------------------------------------------------ layers
# Vectorised over the rows and over the OUTPUT-unit index: the C++ chains run over the
# input index only, so every element still sees its own operations in the source's order.
def _kernels(spec, w):
    """Per-layer kernels as (n, r, c) float32 arrays (copies)."""
    return [w[:, o:o + r * c].reshape(-1, r, c).copy() for (r, c), o in zip(spec.layer_shapes, spec.offsets)]


def _rows(ks):
    return np.concatenate([k.reshape(k.shape[0], -1) for k in ks], axis=1)


def _dense_v(k, x):
    """dense_fwd on k (n, r, c), x (n, r): acc = x0 * k[0], then fma(x_i, k[i], acc)."""
    acc = (x[:, 0:1] * k[:, 0, :]).astype(F32)
    for i in range(1, k.shape[1]):
        acc = fma(x[:, i:i + 1], k[:, i, :], acc)
    return acc


def _chain0(k, d):
    """acc_i = 0; acc_i = fma(k[i][j], d_j, acc_i) over j (cell_bwd's dx and carry)."""
    acc = np.zeros(k.shape[:2], dtype=F32)
    for j in range(k.shape[2]):
        acc = fma(k[:, :, j], d[:, j:j + 1], acc)
    return acc


def _mlp_forward(ks, x):
    acts = [x]
    for k in ks:
        acts.append(_dense_v(k, acts[-1]))
    return acts[-1], acts


def _mlp_step(ks, acts, so):
    """MLP::backward_update from so = -lr * dL/dy: si = K . so (pre-update K, chain from
    k[i][0] * so_0), K[i][j] = fma(x_i, so_j, K[i][j]); layer 0 forms no si."""
    for l in range(len(ks) - 1, -1, -1):
        k = ks[l]
        si = None
        if l > 0:
            si = (k[:, :, 0] * so[:, 0:1]).astype(F32)
            for j in range(1, k.shape[2]):
                si = fma(k[:, :, j], so[:, j:j + 1], si)
        ks[l] = fma(acts[l][:, :, None], so[:, None, :], k)
        so = si


def aggregate(spec: ArchSpec, t) -> np.ndarray:
    """csrc aggregate: mean = sequential double sum / len in double, one cast; max and max_ref
    scan ``v > m`` from the chunk's first weight (max_ref skips zeros: the reference's
    ``weight > max and weight or max``)."""
    t = np.asarray(t, dtype=F32)
    g = np.empty((t.shape[0], spec.aggregates), dtype=F32)
    for k, (s, L) in enumerate(spec.chunks):
        if spec.aggregator == "mean":
            acc = np.zeros(t.shape[0], dtype=F64)
            for i in range(L):
                acc = acc + t[:, s + i].astype(F64)
            g[:, k] = (acc / F64(L)).astype(F32)
        else:
            m = t[:, s].copy()
            for i in range(L):
                v = t[:, s + i]
                m = np.where((v > m) if spec.aggregator == "max" else ((v > m) & (v != 0)), v, m)
            g[:, k] = m
    return g


def _agg_apply(spec, a, t, seed, uids, ctr):
    h, _ = _mlp_forward(_kernels(spec, a), aggregate(spec, t))
    out = np.empty((a.shape[0], spec.P), dtype=F32)
    for k, (s, L) in enumerate(spec.chunks):
        out[:, s:s + L] = h[:, k:k + 1]
    if spec.shuffler == "random":  # shuffle_out: out[k] = tmp[perm[k]]
        out = np.take_along_axis(out, C.fisher_yates(spec.P, seed, uids, ctr, C.P_AGGSHUF), axis=1)
    return out


def _agg_epoch(spec, w, s, lr):
    """Aggregating::train_epoch: one sample x = y = the aggregated weights of ``s``."""
    A = spec.aggregates
    ks = _kernels(spec, w)
    g = aggregate(spec, s)
    h, acts = _mlp_forward(ks, g)
    e = (h - g).astype(F32)
    loss = np.zeros(w.shape[0], dtype=F32)
    for k in range(A):
        loss = fma(e[:, k], e[:, k], loss)
    gy = ((F32(2.0) * e) / F32(A)).astype(F32)
    _mlp_step(ks, acts, (F32(-F32(lr)) * gy).astype(F32))
    return _rows(ks), (loss / F32(A)).astype(F32)


def _rnn_forward(ks, s):
    """Recurrent::apply / the forward half of train_epoch: per step and layer hn = x.K + hp.R
    (two dense_fwd chains, then a plain add).  Returns (out (n, P), hs[t][l])."""
    n, T = s.shape
    nl = len(ks) // 2
    h = [np.zeros((n, ks[2 * l].shape[2]), dtype=F32) for l in range(nl)]
    out = np.empty((n, T), dtype=F32)
    hs = []
    for t in range(T):
        x = s[:, t:t + 1]
        for l in range(nl):
            h[l] = (_dense_v(ks[2 * l], x) + _dense_v(ks[2 * l + 1], h[l])).astype(F32)
            x = h[l]
        hs.append(list(h))
        out[:, t] = x[:, 0]
    return out, hs


def _rnn_epoch(spec, w, s, lr):
    """Recurrent::train_epoch: BPTT over the single (1, P, 1) sample, one SGD step."""
    n, T = w.shape[0], spec.P
    ks = _kernels(spec, w)
    nl = len(ks) // 2
    out, hs = _rnn_forward(ks, s)
    gw = [np.zeros_like(k) for k in ks]
    carry = [np.zeros((n, ks[2 * l].shape[2]), dtype=F32) for l in range(nl)]
    zeros = [np.zeros_like(c) for c in carry]
    loss = np.zeros(n, dtype=F32)
    for t in range(T - 1, -1, -1):
        e = (out[:, t] - s[:, t]).astype(F32)
        loss = fma(e, e, loss)
        dtop = ((F32(2.0) * e) / F32(T)).astype(F32)[:, None]
        hp = hs[t - 1] if t > 0 else zeros
        for l in range(nl - 1, -1, -1):  # bwd_layers / cell_bwd
            K, R = ks[2 * l], ks[2 * l + 1]
            dh = (dtop + carry[l]).astype(F32)
            xin = s[:, t:t + 1] if l == 0 else hs[t][l - 1]
            gw[2 * l] = fma(xin[:, :, None], dh[:, None, :], gw[2 * l])
            gw[2 * l + 1] = fma(hp[l][:, :, None], dh[:, None, :], gw[2 * l + 1])
            if l > 0:
                dtop = _chain0(K, dh)
            carry[l] = _chain0(R, dh)
    ks = [fma(g, F32(-F32(lr)), k) for g, k in zip(gw, ks)]
    return _rows(ks), (loss / F32(T)).astype(F32)


# ------------------------------------------------------------------------------ ops
def apply(spec: ArchSpec, a, t, seed=0, uids=None, ctr=0) -> np.ndarray:
    """f_a(t) per row.  Weightwise: every target weight -> the net's output at its point;
    Aggregating: chunk aggregates -> MLP -> broadcast back (shuffle_random: Fisher-Yates keyed
    by (seed, uids, ctr), as csrc shuffle_out); Recurrent: the weight sequence through the stack."""
    _check(spec)
    a = np.asarray(a, dtype=F32)
    t = np.asarray(t, dtype=F32)
    n = a.shape[0]
    if spec.kind != "weightwise":
        with np.errstate(over="ignore", invalid="ignore"):
            if spec.kind == "recurrent":
                return _rnn_forward(_kernels(spec, a), t)[0]
            return _agg_apply(spec, a, t, seed, np.arange(n, dtype=np.uint64) if uids is None else uids, ctr)
    # every (row, weight) point is one input row of the same net: x = (t_k, layer, cell, pos)
    P = spec.P
    x = np.empty((n, P, 4), dtype=F32)
    x[:, :, 0] = t[:, :P]
    x[:, :, 1:] = spec.coords().astype(F32)[None]
    with np.errstate(over="ignore", invalid="ignore"):
        y, _ = _mlp_forward(_kernels(spec, np.repeat(a[:, :P], P, axis=0)), x.reshape(n * P, 4))
    return y.reshape(n, P)


def _perm(spec, n, shuffle, seed, uids, ctr):
    if not shuffle:
        return np.tile(np.arange(spec.P), (n, 1))
    if spec.P <= 16:
        return C.shuffle16(spec.P, seed, uids, ctr, C.P_SHUFFLE)
    return C.fisher_yates(spec.P, seed, uids, ctr, C.P_SHUFFLE)


def train_epochs(spec: ArchSpec, w, t, epochs: int, self_train: bool, lr=0.01, shuffle=True, seed=0, uids=None,
                 ctr=0):
    """``epochs`` Keras epochs (batch 1) in the engine's order: samples = the weights at each
    epoch start (``self_train``) or the fixed rows ``t`` (learn_from); epoch e permuted with
    counter ``ctr + e``.  Aggregating and Recurrent epochs are one sample each (no SGD shuffle):
    Aggregating::train_epoch / Recurrent::train_epoch.  Returns (w', last epoch's mean loss)."""
    _check(spec)
    w = np.array(w, dtype=F32, copy=True)
    n = w.shape[0]
    if uids is None:
        uids = np.arange(n, dtype=np.uint64)
    if epochs <= 0:
        return w, np.zeros(n, dtype=F32)
    if spec.kind != "weightwise":  # one sample per epoch: no SGD shuffle, the counter only advances
        epoch = _agg_epoch if spec.kind == "aggregating" else _rnn_epoch
        src = None if self_train else np.asarray(t, dtype=F32)
        with np.errstate(over="ignore", invalid="ignore"):
            for _ in range(epochs):
                w, loss = epoch(spec, w, w.copy() if self_train else src, lr)
        return w, loss
    co = spec.coords().astype(F32)
    rows = np.arange(n)
    lr2 = F32(2.0) * F32(lr)
    ks = _kernels(spec, w)
    loss = np.zeros(n, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        src = None if self_train else np.asarray(t, dtype=F32)
        for e in range(epochs):
            s = _rows(ks) if self_train else src  # samples frozen at epoch start
            perm = _perm(spec, n, shuffle, seed, uids, ctr + e)
            acc = np.zeros(n, dtype=F32)
            for q in range(spec.P):
                idx = perm[:, q]
                x = np.empty((n, 4), dtype=F32)
                x[:, 0] = s[rows, idx]
                x[:, 1:] = co[idx]
                y, acts = _mlp_forward(ks, x)
                err = (y[:, 0] - x[:, 0]).astype(F32)
                acc = fma(err, err, acc)
                _mlp_step(ks, acts, (F32(-lr2) * err).astype(F32)[:, None])  # dL/dy = err, lr = 2 lr
            loss = (acc / F32(spec.P)).astype(F32)
    return _rows(ks), loss


# ------------------------------------------------------------------------------ soups
def seq_generation(spec: ArchSpec, W0, gen: int, seed: int, params, lr=0.01, shuffle=True, record_turns=False):
    """One sequential (reference-order, in place) soup generation with the engine's keys
    (csrc Item::soup_seq_one / Ord::turn): slot j in index order attacks att[j] (W[v] =
    f_{W[j]}(W[v]), shuffle_random keyed by the attacker and counter gen * 1024 + 1), learns
    ``learn_from_severity`` epochs from te[j]'s current row, self-trains ``train`` epochs, and is
    re-initialised with respawn_key(gen, j) when divergent / zero.
    Returns (W1, action, counterpart, loss, respawn[, turns]) -- ``turns[j]`` is slot j's row at
    the end of its own turn before any respawn (the per-turn output the tests compare).
    Recurrent nets: only without respawn (no exact init), NotImplementedError otherwise."""
    _check(spec)
    if spec.kind == "recurrent" and (params.get("remove_divergent") or params.get("remove_zero")):
        raise NotImplementedError("no exact init of Recurrent nets: run their generations without respawn")
    n = W0.shape[0]
    att, te = C.soup_decisions(seed, gen, n, params["attacking_rate"], params["learn_from_rate"],
                               int(params.get("segment", 0) or 0))
    W = np.array(W0, dtype=F32, copy=True)
    keys = np.arange(n, dtype=np.uint64)
    action = np.zeros(n, dtype=np.int8)
    cp = np.full(n, -1, dtype=np.int64)
    loss = np.zeros(n, dtype=F32)
    respawn = np.zeros(n, dtype=np.int8)
    turns = np.zeros((n, spec.P), dtype=F32) if record_turns else None
    eps = params.get("epsilon") or 1e-14
    sev = int(params.get("learn_from_severity", 1))
    epochs = int(params.get("train", 0))
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(n):
            v = att[j]
            if v >= 0:
                W[v:v + 1] = apply(spec, W[j:j + 1], W[v:v + 1], seed, keys[j:j + 1], (gen * 1024 + 1) & C.M32)
                action[j], cp[j] = 1, v
            c = (gen * 1024 + 512) & C.M32
            if te[j] >= 0:
                if sev > 0:
                    W[j:j + 1], l = train_epochs(spec, W[j:j + 1], W[te[j]:te[j] + 1], sev, False, lr, shuffle, seed,
                                                 keys[j:j + 1], c)
                    loss[j] = l[0]
                c += sev
                action[j], cp[j] = 2, te[j]
            if epochs > 0:
                W[j:j + 1], l = train_epochs(spec, W[j:j + 1], None, epochs, True, lr, shuffle, seed, keys[j:j + 1], c)
                loss[j] = l[0]
                action[j], cp[j] = 3, -1
            if turns is not None:
                turns[j] = W[j]
            rs = 0
            if params.get("remove_divergent") and C.is_diverged(W[j:j + 1])[0]:
                rs = 1
            elif params.get("remove_zero") and C.is_zero(W[j:j + 1], eps)[0]:
                rs = 2
            if rs:
                W[j] = init(spec, np.array([C.respawn_key(gen, j)], dtype=np.uint64), seed)[0]
            respawn[j] = rs
    out = (W, action, cp, loss, respawn)
    return out + (turns,) if record_turns else out


def max_row_error(a, b) -> float:
    """max over rows of max|a - b| / max(max|b|, 1) (non-finite entries must match)."""
    a = np.asarray(a, dtype=F64)
    b = np.asarray(b, dtype=F64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not np.array_equal(fa, fb):
        return float("inf")
    d = np.where(fa, np.abs(np.where(fa, a, 0) - np.where(fb, b, 0)), 0.0)
    scale = np.maximum(np.max(np.where(fb, np.abs(b), 0.0), axis=1), 1.0)
    return float(np.max(np.max(d, axis=1) / scale)) if a.size else 0.0
