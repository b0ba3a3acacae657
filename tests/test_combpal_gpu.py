"""The PAL Y/C decoder's kernels (csrc/combpal.hip) stage by stage against the oracle
(oracle/combpal.cpp, oracle/comb.py CombPAL) on tests/pal_cases.py's nine frames: SplitIQ's
signed chroma (bit for bit), the burst angles, the V-switch phase, the burst-level EMA
(ldg_debug_read 80..84 after each frame, one frame per call), the rgb48, and the call structure.

The oracle runs once, as one uninterrupted process over the nine frames, in a module fixture;
tests/test_combpal_ref.py shows on the CPU that each frame reaches the decisions it was built
for and that no voted pair of angles is near the vote's threshold.  The angle tolerance is
1000 x the oracle's own floor (pal_cases.FLOOR_ANGLE).
"""
import numpy as np
import pytest

import pal_cases as PC
from oracle.comb import CombPAL

pytestmark = pytest.mark.gpu

WHAT_CV, WHAT_ANGLE, WHAT_PHASE, WHAT_ABL, WHAT_STATE = 80, 81, 82, 83, 84


@pytest.fixture(scope='module')
def chain():
    fr = PC.frames()
    o = CombPAL()
    rgb = o.process(fr, keep_stages=True)
    return dict(frames=fr, rgb=rgb, stages=o.stages, aburstlev=o.aburstlev)


@pytest.fixture(scope='module')
def stepwise(gpu_ctx_ntsc, chain):
    """The GPU over the nine frames, one per call on a reset comb: rgb48 [9, 576, 1057, 3] and
    each call's read-back."""
    ctx, _ = gpu_ctx_ntsc
    ctx.comb_reset()
    try:
        rgb, recs = [], []
        for fr in chain['frames']:
            rgb.append(ctx.comb_pal(fr[None]))
            recs.append(ctx.comb_pal_stages())
        return np.concatenate(rgb), recs
    finally:
        ctx.comb_reset()


@pytest.fixture()
def pal_ctx(gpu_ctx_ntsc):
    ctx, _ = gpu_ctx_ntsc
    ctx.comb_reset()
    yield ctx
    ctx.comb_reset()


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (what, len(bad), [(tuple(b), got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


# ---- SplitIQ's signed chroma -------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(PC.NAMES)), ids=PC.NAMES)
def test_cv_equals_the_oracle(chain, stepwise, k):
    """ldg_k_pal_split against Split1D / Split2D / SplitIQ, bit for bit: the lines whose l - 4
    is below line 24 and whose l + 4 is past the frame (read as zero), the columns before the 2D
    path starts at h = 18, then everything."""
    got, want = stepwise[1][k]['cv'], chain['stages'][k]['cv']
    assert got.shape == (1, PC.CV_ROWS, PC.CV_STRIDE)
    got = got[0]
    assert_same_bits(got[:4], want[:4], 'lines 24..27')
    assert_same_bits(got[618 - PC.SPLIT_L0:], want[618 - PC.SPLIT_L0:], 'lines 618..624')
    assert_same_bits(got[:, 4:18], want[:, 4:18], 'columns 4..17')
    assert_same_bits(got[:, :4], want[:, :4], 'columns 0..3')
    assert_same_bits(got[:, PC.IN_X - 4:], want[:, PC.IN_X - 4:], 'columns 1131..1135')
    assert_same_bits(got, want, 'all')
    assert np.abs(want).max() > 100


# ---- burst angles, vote, burst level -----------------------------------------------------
@pytest.mark.parametrize('k', range(len(PC.NAMES)), ids=PC.NAMES)
def test_burst_angles(chain, stepwise, k):
    got, want = stepwise[1][k]['angle'], chain['stages'][k]['angle']
    assert got.shape == (1, PC.IN_Y)
    got = got[0]
    assert (got[:10] == 0).all() and (want[:10] == 0).all()
    assert ((got >= 0) & (got < 360)).all()
    d = PC.circ_diff(got, want)
    print('%s: max circular |gpu - oracle| %.3g degrees (tolerance %.1e)' % (PC.NAMES[k], d.max(), PC.ANGLE_TOL))
    assert 0 < PC.ANGLE_TOL < 1e-9
    assert d.max() <= PC.ANGLE_TOL, (d.max(), np.argwhere(d > PC.ANGLE_TOL)[:5])
    if PC.NAMES[k] == 'noburst':
        assert (got == 0).all()                      # atan2(0, 0) on every line


@pytest.mark.parametrize('k', range(len(PC.NAMES)), ids=PC.NAMES)
def test_phase(chain, stepwise, k):
    got = stepwise[1][k]['phase']
    assert got.shape == (1,) and got.dtype == np.int32
    assert int(got[0]) == chain['stages'][k]['phase'] == PC.VOTE[PC.NAMES[k]][0]


@pytest.mark.parametrize('k', range(len(PC.NAMES)), ids=PC.NAMES)
def test_burst_level(chain, stepwise, k):
    """The EMA each line used and the state carried on, against the oracle's sequential chain
    (8.0 from the first line: the fixed point ldg_k_pal_angle stops its chain at)."""
    rec = stepwise[1][k]
    assert rec['abl'].shape == (1, PC.ABL_LINES)
    assert_same_bits(rec['abl'][0], chain['stages'][k]['abl'], 'abl')
    assert (rec['abl'] == 8.0).all()
    assert rec['state'] == chain['aburstlev'] == 8.0


# ---- rgb48 -------------------------------------------------------------------------------
def assert_rgb(got, want, what):
    """+-1 everywhere -- the first and last four rows and the columns without Y-NR
    (h >= IN_X - 12) on their own, so that a failure names its edge -- and fewer than
    RGB_DIFF_SHARE of the values differing."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint16, (what, got.shape)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    x0 = PC.IN_X - 12 - 78
    for part, sub in (('rows 0..3', d[..., :4, :, :]), ('rows 572..575', d[..., 572:, :, :]),
                      ('columns from %d' % x0, d[..., :, x0:, :]), ('all', d)):
        assert sub.max() <= 1, (what, part, sub.max(), np.argwhere(sub > 1)[:5])
    assert (d > 0).mean() < PC.RGB_DIFF_SHARE, (what, (d > 0).mean())
    return (d > 0).mean()


@pytest.mark.parametrize('k', range(len(PC.NAMES)), ids=PC.NAMES)
def test_rgb(chain, stepwise, k):
    share = assert_rgb(stepwise[0][k], chain['rgb'][k], PC.NAMES[k])
    print('%s: %.2e of the rgb values differ from the oracle by 1' % (PC.NAMES[k], share))


# ---- call structure ----------------------------------------------------------------------
def test_call_structure(chain, stepwise, pal_ctx):
    """Nine frames in one call (9 > max_frames = 8: ldg_comb_pal's chunk loop), one per call,
    2 + 7: the same bits from the GPU each way, +-1 from the oracle's uninterrupted chain; the
    read-back codes return the last launch's frames, no more."""
    ctx, fr = pal_ctx, chain['frames']
    assert ctx.max_frames == 8 and fr.shape[0] == 9
    whole = ctx.comb_pal(fr)
    last = ctx.comb_pal_stages()                      # the chunk loop's second launch: frame 8 alone
    assert last['phase'].shape == (1,)
    assert_same_bits(last['cv'][0], stepwise[1][8]['cv'][0], 'cv of the last chunk')
    ctx.comb_reset()
    assert ctx.debug(0, WHAT_STATE, np.float64, 1)[0] == -1.0
    split = np.concatenate([ctx.comb_pal(fr[:2]), ctx.comb_pal(fr[2:])])
    assert np.array_equal(whole, stepwise[0]), np.argwhere(whole != stepwise[0])[:5]
    assert np.array_equal(split, stepwise[0]), np.argwhere(split != stepwise[0])[:5]
    for k, name in enumerate(PC.NAMES):
        assert_rgb(whole[k], chain['rgb'][k], name)
    # after 2 + 7: seven frames' worth, whatever the caller has room for
    room = 9
    sizes = {WHAT_CV: PC.CV_ROWS * PC.CV_STRIDE, WHAT_ANGLE: PC.IN_Y, WHAT_PHASE: 1, WHAT_ABL: PC.ABL_LINES}
    got = {w: ctx.debug(0, w, np.int32 if w == WHAT_PHASE else np.float64, room * n) for w, n in sizes.items()}
    assert {w: a.size for w, a in got.items()} == {w: 7 * n for w, n in sizes.items()}
    assert ctx.debug(0, WHAT_STATE, np.float64, room).size == 1
    for j in range(7):
        rec = stepwise[1][2 + j]
        assert_same_bits(got[WHAT_CV].reshape(7, PC.CV_ROWS, PC.CV_STRIDE)[j], rec['cv'][0], ('cv', j))
        assert_same_bits(got[WHAT_ANGLE].reshape(7, PC.IN_Y)[j], rec['angle'][0], ('angle', j))
        assert_same_bits(got[WHAT_ABL].reshape(7, PC.ABL_LINES)[j], rec['abl'][0], ('abl', j))
        assert got[WHAT_PHASE][j] == rec['phase'][0]


def test_readback_codes_need_a_pal_call(chain, stepwise):
    """80..84 say LDG_EINVAL on a context that has not run the PAL decoder; on one that takes
    two frames a chunk, three frames leave the last chunk's single frame to read."""
    from ldgpu import native
    ctx = native.Context('NTSC', 0, max_reads=2)
    try:
        assert ctx.max_frames == 2
        for what in range(80, 85):
            with pytest.raises(native.LDGError):
                ctx.debug(0, what, np.float64, 16)
        assert np.array_equal(ctx.comb_pal(chain['frames'][:3]), stepwise[0][:3])
        rec = ctx.comb_pal_stages()
        assert rec['phase'].tolist() == [PC.VOTE['phase0'][0]] and rec['state'] == 8.0
        assert_same_bits(rec['angle'], stepwise[1][2]['angle'], 'angle of the last chunk')
        for what in (79, 85):
            with pytest.raises(native.LDGError):
                ctx.debug(0, what, np.float64, 16)
    finally:
        ctx.close()
