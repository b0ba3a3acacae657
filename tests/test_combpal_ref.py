"""The PAL Y/C decoder's oracle (oracle/combpal.cpp through oracle/comb.py CombPAL) on
tests/pal_cases.py's inputs, on the CPU: every case reaches the decisions it was built for
(from the stages and branch counters the oracle keeps), no voted pair of burst angles sits at
the vote's 20 degree threshold, the kernel's formulation of the chroma rotation (rotate=True)
agrees with the reference's, the angle floor the GPU tolerance is derived from, and the default
path's rgb48 is still the one the oracle gave before it kept any stages.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import pal_cases as PC
from oracle.comb import CombPAL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pal_cases.json')


@pytest.fixture(scope='module')
def runs():
    """Per case one fresh oracle process on its frame: frame, rgb, stages; rgb_rot with rotate."""
    out = {}
    for name in PC.NAMES:
        fr = PC.CASES[name]()
        o = CombPAL()
        rgb = o.process(fr[None], keep_stages=True)[0]
        assert len(o.stages) == 1
        out[name] = dict(frame=fr, rgb=rgb, rgb_rot=CombPAL(rotate=True).process(fr[None])[0],
                         aburstlev=o.aburstlev, **o.stages[0])
    return out


def test_frames_are_deterministic_and_well_formed():
    a, b = PC.frames(), PC.frames()
    assert a.dtype == np.uint16 and a.shape == (9, PC.IN_Y, PC.IN_X)
    assert np.array_equal(a, b)
    flagged = a[PC.NAMES.index('flagged')]
    for k, name in enumerate(PC.NAMES):
        want = np.full(PC.IN_Y, 32768)
        if name == 'flagged':
            want[list(PC.FLAG_LINES)] = 16384
        assert np.array_equal(a[k][:, 0], want), name
    assert np.array_equal(flagged[:, 1:], a[PC.NAMES.index('offburst')][:, 1:])


@pytest.mark.parametrize('name', PC.NAMES)
def test_vote(runs, name):
    r = runs[name]
    assert (r['phase'], r['phasecount']) == PC.VOTE[name]
    assert len(PC.VOTE_LINES) == 151
    count = sum(abs(r['angle'][l + 1] - r['angle'][l]) < 20 for l in PC.VOTE_LINES)
    assert count == r['phasecount']
    assert r['phase'] == (count > 75)


@pytest.mark.parametrize('name', PC.NAMES)
def test_no_voted_pair_at_the_threshold(runs, name):
    """Then a GPU phase that differs from the oracle's can never be excused by rounding."""
    a = runs[name]['angle']
    gap = min(abs(abs(a[l + 1] - a[l]) - 20) for l in PC.VOTE_LINES)
    print('%s: the closest voted pair is %.3g degrees from the threshold' % (name, gap))
    assert gap >= 1e-6


@pytest.mark.parametrize('name', PC.NAMES)
def test_stage_layout(runs, name):
    r = runs[name]
    assert r['cv'].shape == (PC.CV_ROWS, PC.CV_STRIDE) and r['angle'].shape == (PC.IN_Y,)
    assert not r['cv'][:, :4].any() and not r['cv'][:, PC.IN_X - 4:].any()
    assert not r['angle'][:24].any()                 # lines 0..9 unset, 10..23 atan2(0, 0)
    assert ((r['angle'] >= 0) & (r['angle'] < 360)).all()
    # the burst-level chain sits at its fixed point from the first line on
    assert r['abl'].shape == (PC.ABL_LINES,) and (r['abl'] == 8.0).all() and r['aburstlev'] == 8.0
    # the sums the angles were taken of are the held U / V of this cv
    assert np.array_equal(PC.burst_sums(r['cv']), r['bsum'][PC.SPLIT_L0:])
    assert not r['bsum'][:PC.SPLIT_L0].any()


def test_phase_cases_differ_only_by_the_shift(runs):
    """phase0 and the ties take the other side of the vote with a picture like offburst's."""
    for name in ('phase0', 'tie75', 'tie76'):
        assert runs[name]['counters']['both_zero'] == 0
    # the tie's shifted half votes against, its unshifted half for
    a = runs['tie75']['angle']
    votes = [abs(a[l + 1] - a[l]) < 20 for l in PC.VOTE_LINES]
    assert votes == [l < 320 for l in PC.VOTE_LINES]
    a = runs['tie76']['angle']
    assert [abs(a[l + 1] - a[l]) < 20 for l in PC.VOTE_LINES] == [l < 324 for l in PC.VOTE_LINES]


def test_flagged(runs):
    """invertphase cancels in the rgb; it shows in cv (the sign of the flagged lines) and in
    the burst angle (turned by 180 degrees), hence in the vote."""
    f, o = runs['flagged'], runs['offburst']
    assert np.array_equal(f['rgb'], o['rgb'])
    fl = np.array(PC.FLAG_LINES)
    rest = np.setdiff1d(np.arange(PC.SPLIT_L0, PC.IN_Y), fl)
    assert np.array_equal(f['cv'][fl - PC.SPLIT_L0], -o['cv'][fl - PC.SPLIT_L0])
    assert np.abs(f['cv'][fl - PC.SPLIT_L0]).max() > 100
    assert np.array_equal(f['cv'][rest - PC.SPLIT_L0], o['cv'][rest - PC.SPLIT_L0])
    assert np.abs(PC.circ_diff(f['angle'][fl], o['angle'][fl]) - 180).max() < 1e-9
    assert np.array_equal(f['angle'][rest], o['angle'][rest])
    assert o['phasecount'] - f['phasecount'] == sum(1 for l in PC.VOTE_LINES if (l in fl) != (l + 1 in fl)) == 33


def test_noburst(runs):
    r = runs['noburst']
    assert not r['bsum'].any()
    assert (r['angle'] == 0).all()
    assert np.abs(r['cv'][:, PC.BURST_COLS + 10:]).max() > 100      # the picture does carry chroma


def test_extremes(runs):
    r, n = runs['extremes'], runs['extremes']['counters']
    base = runs['offburst']['counters']
    assert (r['rgb'] == 0).mean() > 0.01 and (r['rgb'] == 65535).mean() > 0.01
    assert (runs['offburst']['rgb'] == 65535).mean() == 0
    assert n['ynr_clamp'] > 10 * base['ynr_clamp'] > 0
    assert n['kn_gt_3kp'] > 0 and base['kn_gt_3kp'] == 0
    assert n['level0'] > 10 * base['level0']         # the base's: the six columns past IN_X - 4 - 2
    assert n['rgb_lo'] > 10 * base['rgb_lo'] and n['rgb_hi'] > 0 and base['rgb_hi'] == 0
    print('extremes: %.1f%% of the rgb values 0, %.1f%% 65535; counters %s' % (
        100 * (r['rgb'] == 0).mean(), 100 * (r['rgb'] == 65535).mean(), n))


def test_edges(runs):
    r, n = runs['edges'], runs['edges']['counters']
    assert n['kn_gt_3kp'] > 0 and n['kp_gt_3kn'] > 0 and n['both_zero_similar'] > 0
    assert n['both_zero'] > n['both_zero_similar']   # and the both-zero pixels that are not similar
    split2d = (PC.IN_Y - 4 + 1 - PC.SPLIT_L0) * (PC.IN_X - 4 - 18)
    assert n['kn_gt_3kp'] + n['kp_gt_3kn'] + n['both_zero'] < split2d      # and the plain branch
    # lines whose l - 4 is below SplitIQ's first line or whose l + 4 is past the frame carry chroma
    assert all(np.abs(r['cv'][k]).max() > 1000 for k in (0, 1, 2, 3, -4, -3, -2, -1))
    # content in the columns where the Y-NR is skipped, and in the first and last output rows
    tail = r['rgb'][:, PC.IN_X - 12 - 78:PC.IN_X - 4 - 78]
    assert tail.std() > 1000 and r['rgb'][:4].std() > 1000 and r['rgb'][-4:].std() > 1000
    print('edges: counters %s' % n)


@pytest.mark.parametrize('name', PC.NAMES)
def test_rotation_as_the_kernel_evaluates_it(runs, name):
    """One sin / cos per row and a 2 x 2 rotation against mag * cis(atan2 + adj)."""
    d = np.abs(runs[name]['rgb'].astype(np.int64) - runs[name]['rgb_rot'].astype(np.int64))
    print('%s: %d of %d rgb values differ between the two formulations' % (name, (d > 0).sum(), d.size))
    assert d.max() <= 1
    assert (d > 0).mean() <= PC.RGB_DIFF_SHARE


def test_floor_angle(runs):
    """The oracle's angles against plain-double degrees(arctan2) of the same sums."""
    worst = {}
    for name in PC.NAMES:
        r = runs[name]
        worst[name] = PC.circ_diff(r['angle'][10:], PC.burst_angles(r['bsum'][10:])).max()
    print('largest circular difference per case: %s' % ' '.join('%s %.3e' % kv for kv in worst.items()))
    assert 0 < max(worst.values()) <= PC.FLOOR_ANGLE
    assert PC.FLOOR_ANGLE <= 2 * max(worst.values())      # the constant is the measurement, not a cushion
    assert PC.ANGLE_TOL == 1000 * PC.FLOOR_ANGLE < 1e-9


def test_default_path_is_the_parents(runs):
    """The stage exports and the rotate flag leave the default path's rgb48 bit for bit."""
    with open(GOLDEN) as f:
        want = json.load(f)['sha256']
    assert sorted(want) == sorted(PC.NAMES)
    got = {name: hashlib.sha256(runs[name]['rgb'].astype('<u2').tobytes()).hexdigest() for name in PC.NAMES}
    assert got == want


def test_stages_of_a_chain_are_those_of_single_frames(runs):
    """One process over all nine frames (what the GPU tests compare with) keeps per-frame stages."""
    o = CombPAL()
    rgb = o.process(PC.frames(), keep_stages=True)
    assert len(o.stages) == 9
    for k, name in enumerate(PC.NAMES):
        assert np.array_equal(rgb[k], runs[name]['rgb'])
        for key in ('cv', 'angle', 'abl'):
            assert np.array_equal(o.stages[k][key], runs[name][key])
        assert o.stages[k]['phase'] == runs[name]['phase']
