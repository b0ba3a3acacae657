"""Inputs of the PAL Y/C decoder's per-stage tests (tests/test_combpal_ref.py on the CPU,
tests/test_combpal_gpu.py on the GPU): one 1135 x 625 uint16 frame per case, pure numpy and
deterministic, each built to reach decisions of the decoder that test_combpal.pal_frame cannot.

The base frame: luma Y_IRE, a 4fsc pattern (a, b, -a, -b)[x % 4] * s(l) with
s(l) = +1 if ((l + shift) // 4) % 2 == 0 else -1 (the shift may apply from a given line on),
the burst vector (a, b) in columns < 200 and five equal-width bars of picture vectors in the
rest, uniform integer noise in [-noise, noise), column 0 = 32768 (16384 on flagged lines).

  locked    the picture carries the burst vector: after the rotation of the burst to 135
            degrees the V-switch flip (U, V) -> (-V, -U) is the identity (what pal_frame gives).
  offburst  the bars: the picture vectors are off the burst's axis, so a wrong flip or a wrong
            phase moves every coloured pixel.
  phase0    shift 3 on every line: lines l, l + 1 (l % 4 == 0) carry opposite signs, the vote
            counts only the burst-less pair 20 / 21: phase 0, count 1.
  tie75     shift 3 from line 320 on: the pairs 20 .. 316 vote, count 75 == tot / 2: phase 0.
  tie76     shift 3 from line 324 on: count 76: phase 1.
  flagged   offburst with column 0 = 16384 on lines 100, 103 .. 298 (invertphase): the rgb is
            offburst's, the burst angle of a flagged line turns by 180 degrees, 33 voted pairs
            hold one flagged line: count 118.
  noburst   burst vector (0, 0), no noise: atan2(0, 0) on every line, every angle exactly 0.
  extremes  blocks of 0 and of 65535, alternate columns 0, column pairs alternating 0 / 65535:
            the level == 0 -> -100 IRE path, the RGB clamps, the Y-NR clamp, kn > 3 kp.
  edges     uniform random uint16 in rows 0..59 and 600..624 and in columns 1080..1134: the
            rows whose l +- 4 neighbours leave the frame, the columns where the Y-NR is
            skipped, all four branches of Split2D's weights.
"""
import numpy as np

from test_combpal import ire_to_u16

IN_X, IN_Y = 1135, 625
OUT_W, OUT_H = 1057, 576
SPLIT_L0, CV_ROWS, CV_STRIDE = 24, 625 - 24, 1136   # the layout of the kernels' cvbuf
FIRST_LINE, ABL_LINES = 44, 579
BURST_H0, BURST_H1 = 100, 132
VOTE_LINES = range(20, IN_Y - 4, 4)                  # 151 pairs (l, l + 1); tot / 2 == 75
Y_IRE = 45.0
BURST = (1100, -600)
BARS = [(300, 1300), (-900, 500), (0, 0), (1500, -900), (-400, -1200)]
BURST_COLS = 200
FLAG_LINES = range(100, 300, 3)

# The largest circular difference (degrees) between the oracle's burst angles -- atan2 in
# double, times 180 / pi in long double, rounded to double (ld-decoder.h's atan2deg) -- and
# np.degrees(np.arctan2(q, i)) of the same sums in plain double, over all cases, as
# test_combpal_ref.test_floor_angle measured it (and measures it again).  The GPU's angles are
# held to MARGIN x this, as the optical-flow tests hold theirs to 1000 x the oracle's own floor:
# 6e-11 degrees, where 20 degrees decide the vote and 1e-3 degrees moves no rgb value.
# Measured 2026-10-20: 5.684e-14 (two ulp of an angle between 128 and 256 degrees) on every case
# with a burst, 0 on noburst.
FLOOR_ANGLE = 5.7e-14
MARGIN = 1000.0
ANGLE_TOL = MARGIN * FLOOR_ANGLE
RGB_DIFF_SHARE = 1e-3                                # the project's cap on rgb values off by 1 LSB


def base_frame(picture=None, burst=BURST, noise=0, seed=0, shift=0, shift_from=0, flagged=()):
    """The base generator (module docstring) as int64, before clipping: picture None -> the bars,
    else one vector for every column from BURST_COLS on."""
    x = np.arange(IN_X)
    vec = np.empty((IN_X, 2), dtype=np.int64)
    vec[:BURST_COLS] = burst
    if picture is None:
        bar = (x[BURST_COLS:] - BURST_COLS) * len(BARS) // (IN_X - BURST_COLS)
        vec[BURST_COLS:] = np.array(BARS, dtype=np.int64)[bar]
    else:
        vec[BURST_COLS:] = picture
    a, b = vec[:, 0], vec[:, 1]
    pat = np.choose(x % 4, [a, b, -a, -b])
    l = np.arange(IN_Y)
    s = np.where(((l + np.where(l >= shift_from, shift, 0)) // 4) % 2 == 0, 1, -1)
    fr = ire_to_u16(Y_IRE) + s[:, None] * pat[None, :]
    if noise:
        fr = fr + np.random.default_rng(seed).integers(-noise, noise, (IN_Y, IN_X))
    fr[:, 0] = 32768
    fr[list(flagged), 0] = 16384
    return fr


def _u16(fr):
    return np.clip(fr, 0, 65535).astype(np.uint16)


def extremes_frame():
    fr = base_frame(noise=100, seed=48)
    x = np.arange(300, 800)
    fr[90:170, 300:800] = 0
    fr[190:270, 300:800] = 65535
    fr[290:370, 300:800:2] = 0
    fr[390:470, 300:800] = np.where((x // 2) % 2 == 0, 0, 65535)[None, :]
    fr[:, 0] = 32768
    return _u16(fr)


# The random rows hold 15 voted pairs whose angles are random; how many of them vote depends on
# the draw.  This seed's draw gives the count 138 that VOTE states (50 and 51 give 136 and 137).
EDGES_SEED = 52


def edges_frame():
    fr = base_frame(noise=100, seed=49)
    rng = np.random.default_rng(EDGES_SEED)
    fr[0:60] = rng.integers(0, 65536, (60, IN_X))
    fr[600:625] = rng.integers(0, 65536, (25, IN_X))
    fr[:, 1080:1135] = rng.integers(0, 65536, (IN_Y, 55))
    fr[:, 0] = 32768
    return _u16(fr)


CASES = {
    'locked': lambda: _u16(base_frame(picture=BURST, noise=250, seed=41)),
    'offburst': lambda: _u16(base_frame(noise=250, seed=42)),
    'phase0': lambda: _u16(base_frame(noise=100, seed=43, shift=3)),
    'tie75': lambda: _u16(base_frame(noise=100, seed=44, shift=3, shift_from=320)),
    'tie76': lambda: _u16(base_frame(noise=100, seed=45, shift=3, shift_from=324)),
    'flagged': lambda: _u16(base_frame(noise=250, seed=42, flagged=FLAG_LINES)),   # offburst + flags
    'noburst': lambda: _u16(base_frame(burst=(0, 0))),
    'extremes': extremes_frame,
    'edges': edges_frame,
}
NAMES = list(CASES)

# phase, phasecount of the V-switch vote per case (exact)
VOTE = {'locked': (1, 151), 'offburst': (1, 151), 'phase0': (0, 1), 'tie75': (0, 75), 'tie76': (1, 76),
        'flagged': (1, 118), 'noburst': (1, 151), 'extremes': (1, 151), 'edges': (1, 138)}


def frames():
    """The nine frames in NAMES' order, (9, 625, 1135) uint16."""
    return np.stack([CASES[n]() for n in NAMES])


def burst_sums(cv):
    """The burst window's sums (i, q) of lines 24..624, [601, 2], from SplitIQ's signed chroma
    cv [601, 1136]: the held U is +cv at h % 4 == 0 and -cv at h % 4 == 2, the held V -cv at
    h % 4 == 1 and +cv at h % 4 == 3, each held over the next pixel; lines from 44 on are read
    two pixels to the right (AdjustY's p[h] = p[h + 2]).  Summed left to right as the decoder does."""
    out = np.zeros((CV_ROWS, 2), dtype=np.float64)
    sh = np.where(np.arange(SPLIT_L0, IN_Y) >= FIRST_LINE, 2, 0)
    rows = np.arange(CV_ROWS)
    for h in range(BURST_H0, BURST_H1):
        p = h + sh
        he = p & ~1
        ho = np.where(p & 1, p, p - 1)
        out[:, 0] += np.where(he % 4 == 0, 1.0, -1.0) * cv[rows, he]
        out[:, 1] += np.where(ho % 4 == 1, -1.0, 1.0) * cv[rows, ho]
    return out


def burst_angles(sums):
    """Degrees in [0, 360) of the sums (i, q) in plain double."""
    a = np.degrees(np.arctan2(sums[..., 1], sums[..., 0]))
    return np.where(a < 0, a + 360.0, a)


def circ_diff(a, b):
    """|a - b| on the circle of 360 degrees."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)
