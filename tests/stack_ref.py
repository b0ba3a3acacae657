"""numpy restatement of the disc stacking rule.  The GPU kernel
(csrc/stack.hip) is held to this file exactly: all arithmetic is integer.  The rule is
build-defined (the snapshot the project follows has no stacker).  Shares only the array
layout with ldgpu/stack.py:

    frames  uint16 [S, F, H, W]      source s, frame f (content ignored where not present)
    present bool   [F, S]
    runs    int16  [F, S, 2, MAX_LINES, 8, 2]   (startx, endx) of field row r of parity p
    counts  int32  [F, S, 2, MAX_LINES]         frame row y is field row y >> 1, parity y & 1
"""
import numpy as np

MAX_LINES = 320
MAX_PER_LINE = 8
OUTW = {'NTSC': 910, 'PAL': 1135}
FRAME_LINES = {'NTSC': 525, 'PAL': 625}
MODES = ('median', 'mean', 'smart-mean')
BIG = 1 << 20                      # sorts after every pixel value


def run_mask(runs, counts, H, W):
    """bool [H, W]: the pixels one source's runs of one frame cover (step 6: a count above 8
    is 8, startx < 0 is 0, endx > W is W)."""
    mask = np.zeros((H, W), dtype=bool)
    for p, r in zip(*np.nonzero(counts > 0)):
        y = 2 * int(r) + int(p)
        if y >= H:
            continue
        for k in range(min(int(counts[p, r]), MAX_PER_LINE)):
            sx, ex = max(int(runs[p, r, k, 0]), 0), min(int(runs[p, r, k, 1]), W)
            if sx < ex:
                mask[y, sx:ex] = True
    return mask


def _rdiv(num, den):
    """(num + den / 2) / den in integer division, 0 where den is 0."""
    safe = np.maximum(den, 1)
    return np.where(den > 0, (num + safe // 2) // safe, 0)


def stack_frame(vals, present, masks, system, combos):
    """One output frame for each (mode, T) of combos.  vals int32 [S, H, W], present bool [S],
    masks bool [S, H, W].  Returns ({(mode, T): uint16 [H, W]}, bool [H, W] residual)."""
    S = vals.shape[0]
    P = np.asarray(present, dtype=bool)
    assert P.any(), 'a frame with no present source is an argument error'
    base = int(np.flatnonzero(P)[0])
    cand = P[:, None, None] & ~masks
    resid = ~cand.any(axis=0)                                  # step 3: C empty -> C = P
    cand |= resid[None] & P[:, None, None]
    m = cand.sum(axis=0)
    key = np.where(cand, vals, BIG)
    v = np.sort(key, axis=0)                                   # the candidates' values first, ascending
    hi = np.take_along_axis(v, (m // 2)[None], axis=0)[0]
    lo = np.take_along_axis(v, np.maximum(m // 2 - 1, 0)[None], axis=0)[0]
    med = np.where(m % 2 == 1, hi, (lo + hi + 1) >> 1)
    total = np.where(cand, vals, 0).sum(axis=0)
    out = {}
    for mode, T in combos:
        if mode == 'median':
            o = med
        elif mode == 'mean':
            o = _rdiv(total, m)
        else:
            K = cand & (np.abs(vals - med[None]) <= T)
            nk = K.sum(axis=0)
            o = np.where(nk > 0, _rdiv(np.where(K, vals, 0).sum(axis=0), nk), med)
        o = o.copy()
        if system == 'NTSC':
            o[:, :2] = vals[base][:, :2]                       # step 2: the burst flag pixels
        assert o.min() >= 0 and o.max() <= 65535
        out[(mode, T)] = o.astype(np.uint16)
    return out, resid


def stack(frames, present, runs, counts, system, combos):
    """{(mode, T): uint16 [F, H, W]} and the residual mask bool [F, H, W]."""
    W, H = OUTW[system], FRAME_LINES[system]
    frames = np.asarray(frames)
    S, F = frames.shape[:2]
    frames = frames.reshape(S, F, H, W)
    present = np.asarray(present, dtype=bool).reshape(F, S)
    outs = {c: np.zeros((F, H, W), dtype=np.uint16) for c in combos}
    resid = np.zeros((F, H, W), dtype=bool)
    for f in range(F):
        masks = np.zeros((S, H, W), dtype=bool)
        if runs is not None:
            for s in range(S):
                if present[f, s]:
                    masks[s] = run_mask(runs[f, s], counts[f, s], H, W)
        o, resid[f] = stack_frame(frames[:, f].astype(np.int32), present[f], masks, system, combos)
        for c in combos:
            outs[c][f] = o[c]
    return outs, resid


def pixel(values, mode, T=3840):
    """The rule on one pixel's candidate values (steps 4): for the hand-computed cases."""
    v = sorted(int(x) for x in values)
    m = len(v)
    med = v[m // 2] if m % 2 else (v[m // 2 - 1] + v[m // 2] + 1) >> 1
    if mode == 'median':
        return med
    if mode == 'mean':
        return (sum(v) + m // 2) // m
    K = [x for x in v if abs(x - med) <= T]
    return (sum(K) + len(K) // 2) // len(K) if K else med
