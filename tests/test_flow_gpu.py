"""The optical-flow kernels (csrc/flow.hip) stage by stage against the oracle
(oracle/farneback.py, oracle/comb.py Comb3DFlow) on tests/flow_cases.py's inputs: the luma
fields (exact), the polynomial expansions at the three pyramid levels, the level-0 flow, the
weight map (ldg_debug_read 70..75 after each frame, one frame per call) and the comb's rgb48
under several call structures.

The flow and expansion tolerances are 1000 x the oracle's own rounding floor, which
test_flow.test_noise_floor measures on the CPU (flow_cases.FLOOR_*); BUILD-DEFINED, parity with
OpenCV unpinned as everywhere in the flow.  The oracle chain runs once per input in a
module fixture (each farneback() is seconds of CPU); no test recomputes it.
"""
import numpy as np
import pytest

import flow_cases as FCS
from oracle import farneback as fb
from oracle.comb import Comb3DFlow

pytestmark = pytest.mark.gpu

DEFAULT = (-1.0, -1.0)
CHAIN_OPTS = {'translate': DEFAULT, 'edges': FCS.NARROW}
WHAT_LUMA, WHAT_EXP0, WHAT_FLOW, WHAT_WEIGHT = 70, 71, 74, 75


def core_range(pair):
    """-c / -r in IRE (negative: the flow path's defaults 0 / 0.5) as the comb scales them."""
    return ((0.0 if pair[0] < 0 else pair[0]) * FCS.IRESCALE, (0.5 if pair[1] < 0 else pair[1]) * FCS.IRESCALE)


@pytest.fixture(scope='module')
def chains():
    """Per input one uninterrupted oracle run: the frames, the rgb48 and per input frame the
    luma fields, flows, weight map and the expansions [level] -> (2, h, w, 5)."""
    out = {}
    for name, pair in CHAIN_OPTS.items():
        fr = FCS.CASES[name]()
        o = Comb3DFlow(*pair, keep_history=True)
        rgb = o.process(fr)
        for h in o.history:
            h['exp'] = None if h['fields'] is None else [
                np.stack([fb.expansion(h['fields'][f], k) for f in range(2)]) for k in range(3)]
        out[name] = dict(frames=fr, rgb=rgb, hist=o.history)
    return out


def read_flow_state(ctx, g):
    """The read-back of the frame just fed (its index g in the comb's run)."""
    rec = dict(fields=None, exp=None, flow=None, weight=None)
    if g >= 1:
        rec['fields'] = ctx.debug(0, WHAT_LUMA, np.uint16, 2 * FCS.FR * FCS.FC).reshape(2, FCS.FR, FCS.FC)
        rec['exp'] = [ctx.debug(0, WHAT_EXP0 + k, np.float64, 2 * h * w * 5).reshape(2, h, w, 5)
                      for k, (h, w) in enumerate(FCS.LEVEL_SHAPES)]
    if g >= 2:
        rec['flow'] = ctx.debug(0, WHAT_FLOW, np.float64, 2 * FCS.FR * FCS.FC * 2).reshape(2, FCS.FR, FCS.FC, 2)
        rec['weight'] = ctx.debug(0, WHAT_WEIGHT, np.float64, FCS.FR * FCS.FC).reshape(FCS.FR, FCS.FC)
    return rec


def run_stepwise(ctx, frames, pair=DEFAULT, **opts):
    """One frame per call on a reset comb with the flow on: (rgb48 frames, per-frame read-backs)."""
    ctx.comb_set_opts(opticalflow=True, **opts)
    try:
        ctx.comb_reset()
        rgb, recs = [], []
        for g in range(frames.shape[0]):
            rgb.append(ctx.comb_ntsc3d(frames[g:g + 1], *pair))
            recs.append(read_flow_state(ctx, g))
        return np.concatenate(rgb), recs
    finally:
        ctx.comb_set_opts()
        ctx.comb_reset()


@pytest.fixture(scope='module')
def gpu_runs(gpu_ctx_ntsc, chains):
    """The GPU on the chains' frames, one frame per call, at each chain's -c / -r and (edges) at
    the defaults too: key (input, pair) -> (rgb48, read-backs)."""
    ctx, _ = gpu_ctx_ntsc
    runs = {}
    for name, pair in list(CHAIN_OPTS.items()) + [('edges', DEFAULT)]:
        runs[name, pair] = run_stepwise(ctx, chains[name]['frames'], pair)
    return runs


# ---- luma fields -------------------------------------------------------------------------
@pytest.mark.parametrize('opts', [dict(), dict(nr_y=0.0), dict(nr_y=20.0), dict(linesout=525)],
                         ids=['default', 'nr_y0', 'nr_y20', 'lines525'])
@pytest.mark.parametrize('name', ['luma', 'translate'])
def test_luma_fields_equal_the_oracle(gpu_ctx_ntsc, name, opts):
    """ldg_k_flow_luma against comb2d_flow_luma + field_images, exactly, for frames 1 and 2 of a
    run (the first frame takes no flow path).  nr_y 0 is raised to 4 raw by the flow path,
    linesout 525 moves firstline from 38 to 20 (rows 23..37 then go through AdjustY / DoYNR)."""
    ctx, _ = gpu_ctx_ntsc
    fr = FCS.CASES[name]()[:3]
    _, recs = run_stepwise(ctx, fr, **opts)
    o = Comb3DFlow(**opts)
    o.lib.comb2d_set_nr_min(o.h, 4.0)                # as Comb3DFlow.process does from its second frame
    for g in (1, 2):
        want = o.luma_fields(fr[g])
        got = recs[g]['fields']
        assert got.dtype == want.dtype == np.uint16
        # field rows whose frame line 23 + f + 2 r is past 524 read 0
        assert (got[0, 251] == 0).all() and (got[1, 251] == 0).all() and (name != 'luma' or want[1, 250].any())
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, opts, g, len(bad), bad[:5])


# ---- expansions --------------------------------------------------------------------------
def rel_diff(got, want):
    return np.abs(got - want) / np.abs(want).max()


@pytest.mark.parametrize('name', ['translate', 'edges'])
def test_expansions(chains, gpu_runs, name):
    """Blur -> resize -> PolyExp at levels 0, 1, 2, both fields, every frame of the run that has
    them, relative to the level's largest coefficient; the 7 outer rows / columns (PolyExp's
    replicated border, n = 7) on their own."""
    _, recs = gpu_runs[name, CHAIN_OPTS[name]]
    worst = [0.0, 0.0, 0.0]
    for g, h in enumerate(chains[name]['hist']):
        if h['exp'] is None:
            assert recs[g]['exp'] is None
            continue
        for k in range(3):
            assert recs[g]['exp'][k].shape == h['exp'][k].shape
            d = rel_diff(recs[g]['exp'][k], h['exp'][k])
            worst[k] = max(worst[k], d.max())
            inner = d[:, 7:-7, 7:-7].max()
            edge = max(d[:, :7].max(), d[:, -7:].max(), d[:, :, :7].max(), d[:, :, -7:].max())
            assert edge <= FCS.EXP_TOL, ('border rows / columns', name, g, k, edge)
            assert inner <= FCS.EXP_TOL, ('interior', name, g, k, inner)
    print('%s expansions: max relative |gpu - oracle| per level %s (tolerance %.1e)' % (
        name, ' '.join('%.2e' % w for w in worst), FCS.EXP_TOL))


# ---- level-0 flow ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['translate', 'edges'])
def test_level0_flow(chains, gpu_runs, name):
    """Every frame with g >= 2: the zero start, the first initial-flow frame and three more."""
    _, recs = gpu_runs[name, CHAIN_OPTS[name]]
    tol = FCS.FLOW_TOL[name]
    assert tol < FCS.FLOW_TOL_CAP
    hist = chains[name]['hist']
    assert [h['flow'] is not None for h in hist] == [False, False, True, True, True, True]
    for g in range(2, 6):
        want, got = np.stack(hist[g]['flow']), recs[g]['flow']
        d = np.abs(got - want)
        ring = np.ones(d.shape, dtype=bool)
        ring[:, 5:-5, 5:-5] = False                  # UpdateMatrices' border scale: the outer 5 pixels
        print('%s frame %d: max |flow| %.3g px, max |gpu - oracle| %.3g px (outer 5 pixels %.3g; tolerance %.1e)' % (
            name, g, np.abs(want).max(), d.max(), d[ring].max(), tol))
        assert d[ring].max() <= tol, ('outer 5 pixels', name, g, d[ring].max())
        assert d.max() <= tol, (name, g, d.max(), np.argwhere(d > tol)[:5])
        if name == 'translate':
            inner = got[:, 48:-48, 96:-96]
            for f in range(2):
                assert np.median(inner[f, ..., 0]) == pytest.approx(FCS.FIELD_FLOW[0], abs=FCS.SHIFT_TOL)
                assert np.median(inner[f, ..., 1]) == pytest.approx(FCS.FIELD_FLOW[1], abs=FCS.SHIFT_TOL)
    if name == 'edges':
        # frame 5 repeats frame 4: no more flow than the oracle's own residue there
        assert np.abs(recs[5]['flow']).max() <= np.abs(np.stack(hist[5]['flow'])).max() + tol


# ---- weight map --------------------------------------------------------------------------
@pytest.mark.parametrize('name,pair', [('translate', DEFAULT), ('edges', DEFAULT), ('edges', FCS.NARROW)],
                         ids=['translate-default', 'edges-default', 'edges-narrow'])
def test_weight_map(chains, gpu_runs, name, pair):
    """ldg_k_flow_combk against the oracle's weights of the oracle's flow, and against the
    formula applied to the flow the GPU itself read back, at the flow tolerance / range."""
    _, recs = gpu_runs[name, pair]
    core, rng = core_range(pair)
    tol = FCS.FLOW_TOL[name] / rng
    hist = chains[name]['hist']
    lo, hi, worst = 1.0, 0.0, 0.0
    for g in range(2, 6):
        want = fb.field_weight(hist[g]['flow'][0], hist[g]['flow'][1], core, rng)
        if pair == CHAIN_OPTS[name]:
            assert np.array_equal(want, hist[g]['weight'])      # what the oracle's comb used
        lo, hi = min(lo, want.min()), max(hi, want.max())
        got = recs[g]['weight']
        own = fb.field_weight(recs[g]['flow'][0], recs[g]['flow'][1], core, rng)
        assert np.abs(got - own).max() <= tol, ('against its own flow', name, pair, g, np.abs(got - own).max())
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got - want).max() <= tol, (name, pair, g, np.abs(got - want).max())
    print('%s -c/-r %s: oracle weights %.3f .. %.3f, max |gpu - oracle| %.3g (tolerance %.1e)' % (
        name, pair, lo, hi, worst, tol))
    if (name, pair) == ('edges', FCS.NARROW):
        assert lo == 0.0 and hi > 0.9                # the weights leave the neighbourhood of 1


# ---- the comb's output under different call structures -----------------------------------
def assert_rgb(got, want, what):
    assert got.shape == want.shape == (4, 480, 744, 3), (what, got.shape)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max() <= 1, (what, d.max(), np.argwhere(d > 1)[:5])


@pytest.fixture()
def flow_ctx(gpu_ctx_ntsc):
    ctx, _ = gpu_ctx_ntsc
    ctx.comb_set_opts(opticalflow=True)
    ctx.comb_reset()
    yield ctx
    ctx.comb_set_opts()
    ctx.comb_reset()


def test_comb_one_frame_per_call(chains, gpu_runs):
    assert_rgb(gpu_runs['edges', FCS.NARROW][0], chains['edges']['rgb'], '1 x 6')


def test_comb_calls_of_1_4_1(chains, flow_ctx):
    fr = chains['edges']['frames']
    parts = [flow_ctx.comb_ntsc3d(fr[a:b], *FCS.NARROW) for a, b in ((0, 1), (1, 5), (5, 6))]
    assert [p.shape[0] for p in parts] == [0, 3, 1]
    assert_rgb(np.concatenate(parts), chains['edges']['rgb'], '1 + 4 + 1')


def test_comb_call_longer_than_max_frames(chains):
    """Six frames in one call on a context that takes two frames a chunk (the comb needs no
    filters set); its flow read-back codes say LDG_EINVAL until a frame took the flow path."""
    from ldgpu import native
    ctx = native.Context('NTSC', 0, max_reads=2)
    try:
        assert ctx.max_frames == 2
        ctx.comb_set_opts(opticalflow=True)
        for what in range(70, 76):
            with pytest.raises(native.LDGError):
                ctx.debug(0, what, np.float64, 16)
        assert_rgb(ctx.comb_ntsc3d(chains['edges']['frames'], *FCS.NARROW), chains['edges']['rgb'], '6 in chunks of 2')
    finally:
        ctx.close()


def test_comb_restart_after_reset(chains, flow_ctx):
    fr = chains['edges']['frames']
    assert flow_ctx.comb_ntsc3d(fr[:3], *FCS.NARROW).shape[0] == 1
    flow_ctx.comb_reset()
    assert_rgb(flow_ctx.comb_ntsc3d(fr, *FCS.NARROW), chains['edges']['rgb'], '3, reset, 6')


def test_comb_flow_after_a_run_without_it(chains, flow_ctx):
    fr = chains['edges']['frames']
    flow_ctx.comb_set_opts(opticalflow=False)
    assert flow_ctx.comb_ntsc3d(fr[:3]).shape[0] == 1          # -d 3 -F
    flow_ctx.comb_set_opts(opticalflow=True)
    flow_ctx.comb_reset()
    assert_rgb(flow_ctx.comb_ntsc3d(fr, *FCS.NARROW), chains['edges']['rgb'], '-F run, flow on, reset, 6')


def test_readback_codes_need_a_flow_frame(chains, flow_ctx):
    """70..73 from the comb's second frame, 74 / 75 from its third, none after comb_reset."""
    from ldgpu import native
    fr = chains['edges']['frames']

    def readable(what):
        try:
            flow_ctx.debug(0, what, np.float64, 16)
            return True
        except native.LDGError:
            return False
    codes = list(range(70, 76))
    assert [readable(w) for w in codes] == [False] * 6
    flow_ctx.comb_ntsc3d(fr[:1], *FCS.NARROW)
    assert [readable(w) for w in codes] == [False] * 6
    flow_ctx.comb_ntsc3d(fr[1:2], *FCS.NARROW)
    assert [readable(w) for w in codes] == [True] * 4 + [False] * 2
    flow_ctx.comb_ntsc3d(fr[2:3], *FCS.NARROW)
    assert [readable(w) for w in codes] == [True] * 6
    assert not readable(76) and not readable(69)
    flow_ctx.comb_reset()
    assert [readable(w) for w in codes] == [False] * 6
