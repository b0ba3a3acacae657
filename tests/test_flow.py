"""The 3D comb with optical flow (comb-ntsc -d 3; comb-ntsc.cxx:600-662,851-858).

BUILD-DEFINED, PARITY UNPINNED: the reference's flow is OpenCV's
calcOpticalFlowFarneback, absent here; oracle/farneback.py restates it (steps,
parameters, borders) in float64.  CPU: closed-form known answers pin that
restatement (no motion gives no flow, a translated pattern gives its shift, the
weight map's formula).  GPU: csrc/flow.hip through the comb within +-1 LSB of
the oracle's comb (oracle/comb.py Comb3DFlow); stage by stage in tests/test_flow_gpu.py,
whose inputs (tests/flow_cases.py) and tolerances the CPU tests at the end of this file pin.
"""
import numpy as np
import pytest

import flow_cases as FCS
from flow_cases import pattern
from oracle import farneback as fb


def test_no_motion_gives_no_flow():
    a = pattern()
    f = fb.farneback(a, a)
    # exactly 0 away from the edges; the edge rows / columns (OpenCV's 'outside' branch of
    # UpdateMatrices) leave a small residue within the 61-pixel box
    assert np.abs(f).max() < 0.05
    assert np.abs(f[64:-64, 128:-128]).max() < 1e-3


@pytest.mark.parametrize('dy,dx', [(0, 3), (-2, 0), (1, -2)])
def test_translation_gives_its_shift(dy, dx):
    """calcOpticalFlowFarneback(prev, next): prev(y, x) = next(y + fy, x + fx); a pattern
    moved by (dy, dx) from next to prev gives flow (-dx, -dy) in the interior."""
    a = pattern(seed=2)
    b = np.roll(a, (dy, dx), axis=(0, 1))
    f = fb.farneback(b, a)
    inner = f[48:-48, 96:-96]
    assert np.median(inner[..., 0]) == pytest.approx(-dx, abs=1e-3)
    assert np.median(inner[..., 1]) == pytest.approx(-dy, abs=1e-3)


def test_initial_flow_converges_to_the_same_shift():
    a = pattern(seed=3)
    b = np.roll(a, 2, axis=1)
    f0 = fb.farneback(b, a)
    f1 = fb.farneback(b, a, f0)           # OPTFLOW_USE_INITIAL_FLOW (the reference's third call on)
    assert np.median(f1[48:-48, 96:-96, 0]) == pytest.approx(-2, abs=1e-3)


def test_weight_map_formula():
    """c = 1 - clamp((|(fy, 2 fx)| - core) / range, 0, 1), the smaller field, rows 2y / 2y+1,
    columns 70..909 (comb-ntsc.cxx:633-650); 0 elsewhere."""
    f0 = np.zeros((252, 840, 2))
    f1 = np.zeros((252, 840, 2))
    f0[..., 0] = 30.0                   # |(0, 60)| = 60
    f1[..., 1] = 20.0                   # |(20, 0)| = 20
    k = fb.combk_from_flow(f0, f1, 0.0, 179.2)
    assert k.shape == (525, 910)
    assert k[0, 70] == pytest.approx(1 - 60 / 179.2) and k[503, 909] == k[0, 70]
    assert (k[504:] == 0).all() and (k[:, :70] == 0).all()


def test_gaussian_kernels():
    assert fb.gaussian_kernel(3, 0).tolist() == [0.25, 0.5, 0.25]
    k = fb.gaussian_kernel(9, 1.5)
    assert k.sum() == pytest.approx(1.0) and k[4] == k.max() and np.allclose(k, k[::-1])


# ---- tests/flow_cases.py: the inputs and tolerances of the per-stage GPU tests ------------
@pytest.fixture(scope='module')
def case_chains():
    """The oracle's comb over translate (3 frames: one flow) and edges (5 frames: the zero start,
    the cut, the frame after it), with UpdateMatrices' sampling positions watched: per call the
    level's shape and how many pixels off the last row and column (which sample outside at any
    flow) took the `outside` branch."""
    from oracle.comb import Comb3DFlow
    outside = {}
    orig = fb.update_matrices

    def watched(R0, R1, flow):
        h, w = flow.shape[:2]
        x1 = np.floor(np.arange(w)[None, :] + flow[..., 0])
        y1 = np.floor(np.arange(h)[:, None] + flow[..., 1])
        out = (x1 < 0) | (x1 >= w - 1) | (y1 < 0) | (y1 >= h - 1)
        outside.setdefault(name, []).append(((h, w), int(out[:-1, :-1].sum())))
        return orig(R0, R1, flow)
    chains = {}
    fb.update_matrices = watched
    try:
        for name, n in (('translate', 3), ('edges', 5)):
            o = Comb3DFlow(*FCS.NARROW, keep_history=True)
            o.process(FCS.CASES[name]()[:n])
            chains[name] = o.history
    finally:
        fb.update_matrices = orig
    return chains, outside


def test_cases_are_what_they_say():
    """The frames' construction: shapes, the repeated last frame of edges, the cut, and that
    luma reaches what ldg_k_flow_luma has to get right (see flow_cases' docstring)."""
    fr = {k: f() for k, f in FCS.CASES.items()}
    assert fr['translate'].shape == fr['edges'].shape == (6, 525, 910) and fr['luma'].shape == (3, 525, 910)
    assert all(f.dtype == np.uint16 for f in fr.values())
    assert np.array_equal(fr['edges'][5], fr['edges'][4]) and not np.array_equal(fr['edges'][4], fr['edges'][3])
    lu = fr['luma']
    assert set(np.unique(lu[:, :, 0])) == {16384, 32768}
    assert (lu[:, 38:522, 210:250] == 0).mean() > 0.4 and (lu[:, 38:522, 310:350] == 65535).mean() > 0.4
    # so the flow path's luma (a double) leaves 0..65535 both ways before it goes to uint16
    from oracle.comb import Comb3DFlow
    o = Comb3DFlow()
    o.lib.comb2d_set_nr_min(o.h, 4.0)
    y = np.zeros((525, 910))
    o.lib.comb2d_flow_luma(o.h, np.ascontiguousarray(lu[2]).ctypes.data, y.ctypes.data)
    assert y[38:, 70:].min() < -1000 and y[38:, 70:].max() > 66000
    assert o.luma_fields(lu[2])[1, 250].any() and not o.luma_fields(lu[2])[:, 251].any()
    assert lu[:, 522:525, 70:].std() > 10000
    assert np.abs(np.diff(lu[:, 100:500, 66:75].astype(np.int64), axis=2)).min() > 10000
    assert np.abs(np.diff(lu[:, 100:500, 905:910].astype(np.int64), axis=2)).min() > 10000
    assert FCS.SHIFT[0] % 2 == 0 and FCS.SHIFT[0] and FCS.SHIFT[1]


def test_translate_case_gives_its_shift(case_chains):
    """test_translation_gives_its_shift through the real luma-field path (chroma, AdjustY,
    DoYNR, uint16): both fields' median interior flow is the shift in field rows and columns."""
    h = case_chains[0]['translate'][2]
    for f in range(2):
        inner = h['flow'][f][48:-48, 96:-96]
        assert np.median(inner[..., 0]) == pytest.approx(FCS.FIELD_FLOW[0], abs=FCS.SHIFT_TOL)
        assert np.median(inner[..., 1]) == pytest.approx(FCS.FIELD_FLOW[1], abs=FCS.SHIFT_TOL)


def test_edges_case_reaches_the_branches(case_chains):
    """edges: x + flow leaves the image at levels 0 and 1 (UpdateMatrices' `outside` branch off
    the last row / column), the cut leaves a large flow as the next frame's initial estimate,
    and at -c / -r = NARROW the weights span 0 .. above 0.9; at the defaults they stay above
    0.25 (1 - 24 / 179.2 = 0.87 for the 12-column flow)."""
    chains, outside = case_chains
    for shape in FCS.LEVEL_SHAPES[:2]:
        assert max(n for s, n in outside['edges'] if s == shape) > 0, shape
    hist = chains['edges']
    assert [h['flow'] is not None for h in hist] == [False, False, True, True, True]
    assert np.abs(np.stack(hist[3]['flow'])).max() > 30           # the cut: meaningless, large
    inner = hist[4]['flow'][0][48:-48, 96:-200]
    assert np.median(inner[..., 0]) == pytest.approx(FCS.EDGES_DX, abs=0.05)
    w = np.stack([h['weight'] for h in hist[2:]])
    assert w.min() == 0.0 and w.max() > 0.9 and 0.05 < (w < 0.5).mean() < 0.95
    wd = np.stack([fb.field_weight(h['flow'][0], h['flow'][1], 0.0, 0.5 * FCS.IRESCALE) for h in hist[2:]])
    assert wd.min() > 0.25 and np.median(wd) > 0.8


def test_noise_floor(case_chains):
    """The tolerances of tests/test_flow_gpu.py: the oracle's own rounding floor on one frame
    pair of translate (zero start) and the later edges pair (after the cut, with an initial
    flow), top field.  The flow is computed as it stands, with box_sum as the sequential running
    sums of ldg_k_flow_vsum / ldg_k_flow_hsum_solve (OpenCV's order), and with poly_exp's
    output moved by one ulp at random; the floor is the largest difference among the three
    (expansions: the jittered against the plain ones, relative to the level's largest
    coefficient).  flow_cases' constants must cover it, and 1000 x the floor must stay below
    FLOW_TOL_CAP.  Measured 2026-10-20: see flow_cases.FLOOR_FLOW."""
    chains = case_chains[0]
    orig_box, orig_poly = fb.box_sum, fb.poly_exp
    for name, g in (('translate', 2), ('edges', 4)):
        hist = chains[name]
        cur, prev = hist[g]['fields'][0], hist[g - 1]['fields'][0]
        init = hist[g - 1]['flow'][0] if g >= 3 else None
        base = hist[g]['flow'][0]
        plain = [fb.expansion(cur, k) for k in range(3)]
        try:
            fb.box_sum = FCS.box_sum_running
            run = fb.farneback(cur, prev, init)
            fb.box_sum = orig_box
            fb.poly_exp = FCS.ulp_jitter(orig_poly, 7)
            jit = fb.farneback(cur, prev, init)
            jexp = [fb.expansion(cur, k) for k in range(3)]
        finally:
            fb.box_sum, fb.poly_exp = orig_box, orig_poly
        d_run, d_jit, d_rj = (np.abs(a - b).max() for a, b in ((run, base), (jit, base), (run, jit)))
        floor = max(d_run, d_jit, d_rj)
        efloor = [np.abs(a - b).max() / np.abs(b).max() for a, b in zip(jexp, plain)]
        print('%s frames %d -> %d: max |flow| %.3g px; running sums %.3g px, 1-ulp jitter %.3g px, floor %.3g px '
              '(constant %.3g); expansions %s (constant %.3g)' % (
                  name, g - 1, g, np.abs(base).max(), d_run, d_jit, floor, FCS.FLOOR_FLOW[name],
                  ' '.join('%.3g' % e for e in efloor), FCS.FLOOR_EXP))
        assert 0 < floor <= FCS.FLOOR_FLOW[name]
        assert 0 < max(efloor) <= FCS.FLOOR_EXP
        assert FCS.FLOW_TOL[name] == 1000 * FCS.FLOOR_FLOW[name] < FCS.FLOW_TOL_CAP == 1e-6
    assert FCS.EXP_TOL == 1000 * FCS.FLOOR_EXP


def test_running_box_sum_is_the_box_sum():
    """The restatement the floor is measured with is the same sum in another order."""
    rng = np.random.default_rng(5)
    M = rng.uniform(-1, 1, (70, 90, 5))
    assert np.abs(FCS.box_sum_running(M, 30) - fb.box_sum(M, 30)).max() < 1e-11


def test_expansion_is_the_level_farneback_uses():
    """oracle.farneback.expansion(img, k): blur -> resize -> poly_exp with level k's sigma and
    size, the shapes the GPU keeps per level."""
    a = pattern(seed=4)
    for k, shape in enumerate(FCS.LEVEL_SHAPES):
        scale, sigma, smooth, w, h = fb.level_params(k, *a.shape)
        assert (h, w) == shape and scale == 0.5 ** k
        img = fb.gaussian_blur(a, smooth, sigma)
        if k:
            img = fb.resize_linear(img, w, h)
        assert np.array_equal(fb.expansion(a, k), fb.poly_exp(img))
    assert fb.pyramid_levels(*a.shape) == 2


@pytest.mark.gpu
@pytest.mark.parametrize('opts', [dict(), dict(black_ire=0.0, nr_c=1.0)])
def test_gpu_comb3d_optical_flow_matches_oracle(gpu_ctx_ntsc, opts):
    """The GPU flow (csrc/flow.hip) inside the 3D comb against the oracle's, +-1 LSB, in calls
    of 2 and 3 frames (the flow and the held frames cross the call boundary)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_comb import frames_3d
    from oracle.comb import Comb3DFlow
    ctx, _ = gpu_ctx_ntsc
    fr = frames_3d(seed=19, n=5)
    ctx.comb_set_opts(opticalflow=True, **opts)
    try:
        ctx.comb_reset()
        g = np.concatenate([ctx.comb_ntsc3d(fr[:2]), ctx.comb_ntsc3d(fr[2:])])
        o = Comb3DFlow(**opts).process(fr)
        assert g.shape == o.shape == (3, 480, 744, 3)
        d = np.abs(g.astype(np.int64) - o.astype(np.int64))
        assert d.max() <= 1, (d.max(), np.argwhere(d > 1)[:5])
    finally:
        ctx.comb_set_opts()
        ctx.comb_reset()
