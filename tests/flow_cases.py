"""Inputs of the optical-flow tests (tests/test_flow.py on the CPU, tests/test_flow_gpu.py
on the GPU): 525 x 910 uint16 frames built as test_comb.frames_3d builds them (alternating-
phase chroma from frame_solid, burst columns, the phase flag in column 0) with the luma
replaced, the tolerances the GPU tests use, and the restatements the noise-floor test
perturbs the oracle with.

  translate  6 frames: a smooth texture between about 10 and 90 IRE moved by SHIFT (frame
             rows, columns) per frame, no noise.  Well conditioned; the interior flow of a
             field is the shift in field rows and columns, (-dx, -dy / 2).
  edges      6 frames: the texture moves 12 columns a frame (flow x +12: x + dx leaves the
             image at levels 0 and 1, UpdateMatrices' `outside` branch), a little noise;
             frame 3 cuts to an unrelated texture (a large meaningless flow becomes the
             next frame's initial estimate); frame 5 is frame 4 again (flow 0).
  luma       3 frames for the luma-field kernel alone: flat columns at 0 and 65535 and a
             4-sample 0 / 65535 stripe (Y - clip leaves 0..65535 both ways: the conversion
             to uint16 wraps), strong edges at columns 66..74 and 905..909 (the ends of
             DoYNR's 25-tap window around the first and last column the flow reads), content
             on rows 522..524 (field rows from frame line 525 on read 0), lines with and
             without the 16384 phase flag.
"""
import numpy as np

from test_comb import frame_solid, ire_to_u16

FR, FC = 252, 840                       # a field of the flow
LEVEL_SHAPES = [(252, 840), (126, 420), (63, 210)]
SHIFT = (2, -3)                         # translate: frame rows, columns per frame
FIELD_FLOW = (-SHIFT[1], -SHIFT[0] / 2)   # its interior flow (x, y) in field pixels
EDGES_DX = 12
TEXTURE_ZOOM = 4                        # pattern() magnified (cubic): see fade()
TEXTURE_IRE = {'translate': (35.0, 65.0), 'edges': (46.0, 54.0), 'luma': (10.0, 90.0)}
EDGES_NOISE = 4
# -c / -r (IRE) at which the oracle's weights on `edges` span 0 .. above 0.9 (asserted on the CPU)
NARROW = (0.002, 0.03)
IRESCALE = 358.4

# The oracle's own rounding floor (test_flow.test_noise_floor measures it and asserts that these
# cover it): the largest change of the level-0 flow (px) and of the expansions (relative to the
# level's largest coefficient) when the 61-tap box sums run as OpenCV's sequential running sums
# or the expansions move by 1 ulp (top field of one frame pair).  Measured 2026-10-20:
#                                                running sums   1-ulp jitter   expansions (levels 0 1 2)
#   translate frames 1 -> 2 (zero start)         5.2e-10 px     6.0e-14 px     2.5e-16 2.6e-16 1.5e-16
#   edges frames 3 -> 4 (initial flow: the cut)  5.4e-10 px     3.6e-13 px     2.7e-16 2.8e-16 1.6e-16
# The running-sum figure is 1e-14 px over the picture and reaches 5e-10 only in the columns
# where the picture runs out into the flow path's dead band (see fade()).
FLOOR_FLOW = {'translate': 8e-10, 'edges': 8e-10}
FLOOR_EXP = 4e-16
SHIFT_TOL = 1e-3                        # px: translate's median interior flow against SHIFT
# The GPU tolerance is 1000 x the floor: the experiment perturbs one stage by 1 ulp, the kernels
# differ from NumPy in summation order in every stage of three levels and three iterations.
MARGIN = 1000.0
FLOW_TOL = {k: MARGIN * v for k, v in FLOOR_FLOW.items()}
EXP_TOL = MARGIN * FLOOR_EXP
FLOW_TOL_CAP = 1e-6                     # px: far below any algorithmic error (0.01 px moves 1 LSB)


def pattern(seed=1, shape=(252, 840)):
    """A smooth random texture (8-pixel blocks blurred): the flow has structure to lock on."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    a = np.kron(rng.uniform(0, 60000, (shape[0] // 8 + 1, shape[1] // 8 + 1)), np.ones((8, 8)))[:shape[0], :shape[1]]
    return gaussian_filter(a, 3)


def _ramp(n, lo, hi):
    """0 up to index lo, a raised-cosine rise to 1 at index hi (lo > hi: a fall)."""
    t = np.clip((np.arange(n, dtype=np.float64) - lo) / (hi - lo), 0.0, 1.0)
    return 0.5 - 0.5 * np.cos(np.pi * t)


def fade():
    """The picture fades to 0 over 32 field rows / 64 columns towards the places where the
    flow path's luma is 0 whatever the frame holds: lines below 38 (SplitIQ / AdjustY start),
    lines from 525 on, and columns from 842 on (field columns 772..839: the dead band).

    Why the inputs look as they do.  Where the picture runs out into the dead band the box
    sums G fall through the 1e-3 regulariser of the 2 x 2 solve.  A running sum arrives there
    with the rounding residue of the picture it has passed (eps x the interior's sums), which
    a direct sum does not have, and the solve divides that residue by ~1e-3.  Measured on the
    oracle (running sums against direct sums, zero start): a 10..90 IRE texture of pattern()'s
    own scale gives 7.6e-8 px with the step left in and 3.7e-8 px faded, against 1e-14 px
    over the picture; +-250 noise and the 12-column motion give 1.1e-7.  The GPU tolerance is
    1000 x that and has to stay below FLOW_TOL_CAP, so the inputs are made milder, not the
    cap wider: the texture is pattern() magnified TEXTURE_ZOOM times, its contrast is
    TEXTURE_IRE (translate 30 IRE, edges 8 IRE), the noise of edges is +-EDGES_NOISE, and the
    picture fades instead of stepping.  The branches the kernels take depend on the flow's
    geometry, not on the contrast."""
    rows = _ramp(525, 38, 102) * _ramp(525, 524, 460)
    cols = _ramp(910, 840, 776)
    return rows[:, None] * cols[None, :]


def _compose(luma, k, window=None):
    """Frame k: the luma image (525 x 910, uint16 units) plus frames_3d's chroma, times the
    window if any, and the burst columns."""
    s = 1 if k % 2 == 0 else -1
    chroma = frame_solid(45.0, s * 1100, -s * 600).astype(np.int64) - ire_to_u16(45.0)
    fr = luma + chroma
    if window is not None:
        fr = fr * window
    fr = np.rint(fr).astype(np.int64)
    fr[:, :2] = frame_solid(45.0, burst_ire=20.0 + k)[:, :2]
    return np.clip(fr, 0, 65535).astype(np.uint16)


def _canvas(seed, case):
    """A texture larger than a frame, about 10..90 IRE; frame rows in pairs, so that a shift by
    two frame rows is one field row in both fields."""
    from scipy.ndimage import zoom
    t = zoom(pattern(seed, (360 // TEXTURE_ZOOM, 1100 // TEXTURE_ZOOM)), TEXTURE_ZOOM, order=3)
    lo, hi = (ire_to_u16(v) for v in TEXTURE_IRE[case])
    return np.repeat(lo + t * ((hi - lo) / 60000.0), 2, axis=0)


def _crop(canvas, oy, ox):
    return canvas[oy:oy + 525, ox:ox + 910]


def translate_frames():
    c = _canvas(31, 'translate')
    w = fade()
    return np.stack([_compose(_crop(c, 40 - SHIFT[0] * k, 60 - SHIFT[1] * k), k, w) for k in range(6)])


def edges_frames():
    a, b = _canvas(32, 'edges'), _canvas(33, 'edges')
    rng = np.random.default_rng(34)
    w = fade()
    out = []
    for k in range(5):
        c = a if k < 3 else b
        out.append(_compose(_crop(c, 40, 20 + EDGES_DX * k) + rng.integers(-EDGES_NOISE, EDGES_NOISE, (525, 910)), k, w))
    out.append(out[-1].copy())
    return np.stack(out)


def luma_frames():
    rng = np.random.default_rng(35)
    out = []
    for k in range(3):
        y = _crop(_canvas(36 + k, 'luma'), 40, 60).copy()
        y[:, 200:260] = 0
        y[:, 300:360] = 65535
        y[:, 400:460] = np.where(np.arange(60) % 4 < 2, 0, 65535)[None, :]
        y[:, 520:524] = 65535                      # one chroma-period pulse on a mid grey
        y[:, 66:75] += np.array([9000, -9000, 12000, -12000, 15000, -15000, 12000, -9000, 9000]) * (1 + k)
        y[:, 905:910] += np.array([-14000, 14000, -14000, 14000, -14000])
        y[522:525] = rng.integers(0, 65536, (3, 910))
        y += rng.integers(-250, 250, (525, 910))
        out.append(_compose(np.clip(y, 0, 65535), k))
    return np.stack(out)


CASES = {'translate': translate_frames, 'edges': edges_frames, 'luma': luma_frames}


# ---- the noise-floor experiment's restatements ------------------------------------------
def box_sum_running(M, m):
    """farneback.box_sum as FarnebackUpdateFlow_Blur (and ldg_k_flow_vsum /
    ldg_k_flow_hsum_solve) computes it: a running sum down each column, then along each row,
    started as v = s[0] * (m + 2) + s[1] + .. + s[m - 1] and moved by
    v += s[clamp(y + m)] - s[clamp(y - m - 1)] before each output."""
    def run(a):                                    # along axis 0
        n = a.shape[0]
        cl = lambda i: min(max(i, 0), n - 1)       # noqa: E731
        v = a[0] * (m + 2)
        for y in range(1, m):
            v = v + a[cl(y)]
        out = np.empty_like(a)
        for y in range(n):
            v = v + (a[cl(y + m)] - a[cl(y - m - 1)])
            out[y] = v
        return out
    v = run(np.asarray(M, dtype=np.float64))
    return run(v.transpose(1, 0, 2)).transpose(1, 0, 2)


def ulp_jitter(poly_exp, seed):
    """poly_exp with its output times 1 + u 2^-52, u in {-1, 0, 1} from a seeded generator."""
    rng = np.random.default_rng(seed)

    def jittered(src, *a, **kw):
        r = poly_exp(src, *a, **kw)
        return r * (1.0 + rng.integers(-1, 2, r.shape) * 2.0 ** -52)
    return jittered
