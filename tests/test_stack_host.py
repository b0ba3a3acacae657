"""The disc stacker's host side without a GPU: the numpy restatement of the rule
(tests/stack_ref.py) on hand-computed pixels, ldgpu/stack.py's alignment, run arrays and
residual, disc_stacker.py's refusals, and the library's new exports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stack_ref as R
from ldgpu import stack as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, 'ld-decode_amd', 'disc_stacker.py')


# ---- the restatement on hand-computed cases ------------------------------------------------
def one_pixel(values, system='PAL', masked=(), absent=(), x=5, mode='smart-mean', T=3840):
    """stack_ref.stack on frames that hold values[s] at (row 3, x); masked: sources with a
    one-pixel run there."""
    n = len(values)
    W, H = R.OUTW[system], R.FRAME_LINES[system]
    frames = np.zeros((n, 1, H, W), dtype=np.uint16)
    runs = np.zeros((1, n, 2, R.MAX_LINES, 8, 2), dtype=np.int16)
    counts = np.zeros((1, n, 2, R.MAX_LINES), dtype=np.int32)
    for s, v in enumerate(values):
        frames[s, 0, 3, x] = v
    for s in masked:
        runs[0, s, 1, 1, 0] = (x, x + 1)                 # frame row 3 = field row 1 of parity 1
        counts[0, s, 1, 1] = 1
    present = np.ones((1, n), dtype=bool)
    present[0, list(absent)] = False
    out, resid = R.stack(frames, present, runs, counts, system, [(mode, T)])
    return int(out[(mode, T)][0, 3, x]), bool(resid[0, 3, x])


def test_rule_odd_and_even_counts():
    assert one_pixel([10, 50, 20], mode='median') == (20, False)
    assert one_pixel([10, 50, 20, 41], mode='median') == (31, False)        # (20 + 41 + 1) >> 1
    assert one_pixel([10, 50, 20], mode='mean') == (27, False)              # (80 + 1) // 3
    assert one_pixel([10, 50, 20, 41], mode='mean') == (30, False)          # (121 + 2) // 4
    assert one_pixel([1, 2], mode='mean') == (2, False)                     # (3 + 1) // 2
    assert one_pixel([7], mode='median')[0] == one_pixel([7], mode='mean')[0] == one_pixel([7])[0] == 7


def test_rule_smart_mean_thresholds():
    assert one_pixel([0, 65535], T=0) == (32768, False)                     # K empty: the median
    assert one_pixel([0, 65535], T=32767) == (65535, False)                 # 32768 - 0 > T, 65535 - 32768 = T: K = {65535}
    assert one_pixel([0, 65535], T=32768)[0] == 32768                       # both within: (65535 + 1) // 2
    assert one_pixel([100, 110, 5000], T=0)[0] == 110                       # only the median itself
    assert one_pixel([100, 110, 5000], T=10)[0] == 105
    assert one_pixel([100, 110, 5000], T=65535)[0] == (5210 + 1) // 3
    assert one_pixel([100, 104, 108, 60000], T=3840)[0] == 104              # median 106; the outlier leaves
    assert R.pixel([0, 65535], 'smart-mean', 0) == 32768 and R.pixel([100, 104, 108, 60000], 'smart-mean') == 104


def test_rule_masks_residual_and_absent():
    assert one_pixel([100, 60000, 104], masked=[1], mode='mean') == (102, False)
    assert one_pixel([100, 60000, 104], masked=[0, 1, 2], mode='median') == (104, True)    # C = P
    assert one_pixel([100, 60000, 104], masked=[0, 2], mode='median') == (60000, False)
    assert one_pixel([100, 60000, 104], absent=[1], mode='mean') == (102, False)
    assert one_pixel([100, 60000, 104], absent=[0], masked=[1], mode='mean') == (104, False)
    assert one_pixel([100, 60000, 104], absent=[0], masked=[1, 2], mode='mean') == (30052, True)


def test_rule_ntsc_burst_flag_pixels():
    # x < 2: base's pixel, masked or not; base is the lowest-index present source
    assert one_pixel([100, 60000, 104], system='NTSC', x=1, masked=[0], mode='median') == (100, False)
    assert one_pixel([100, 60000, 104], system='NTSC', x=0, absent=[0], masked=[1], mode='median')[0] == 60000
    assert one_pixel([100, 60000, 104], system='NTSC', x=2, masked=[0], mode='median')[0] == 30052
    assert one_pixel([100, 60000, 104], system='PAL', x=1, masked=[0], mode='median')[0] == 30052


def test_rule_clamps_counts_and_bounds():
    W, H = R.OUTW['PAL'], R.FRAME_LINES['PAL']
    runs = np.zeros((2, R.MAX_LINES, 8, 2), dtype=np.int16)
    counts = np.zeros((2, R.MAX_LINES), dtype=np.int32)
    runs[0, 312, 0] = (-7, 3)
    runs[0, 312, 1] = (W - 2, W + 9)
    counts[0, 312] = 11                                   # read as 8; runs 2..7 are empty
    m = R.run_mask(runs, counts, H, W)
    assert m.sum() == 5 and m[624, :3].all() and m[624, W - 2:].all()


# ---- align ---------------------------------------------------------------------------------
def meta(keys):
    return [{'frame': i, 'vbi': {'framenr': k}, 'fields': []} for i, k in enumerate(keys)]


def test_align_by_frame_number():
    a, b, c = meta([10, 11, 12, 13]), meta([12, 13, 14]), meta([None, 11, 11, 13, 15])
    frames, skipped = S.align([a, b, c])
    assert frames == [(10, [0, None, None]), (11, [1, None, 1]), (12, [2, 0, None]), (13, [3, 1, 3]),
                      (14, [None, 2, None]), (15, [None, None, 4])]
    assert skipped == [{'no_key': 0, 'repeated': 0}, {'no_key': 0, 'repeated': 0}, {'no_key': 1, 'repeated': 1}]
    assert [k for k, _ in S.align([a, b, c], min_sources=2)[0]] == [11, 12, 13]
    assert [k for k, _ in S.align([a, b, c], min_sources=3)[0]] == [13]
    assert [k for k, _ in S.align([a, b, c], start=12, length=2)[0]] == [12, 13]
    assert [k for k, _ in S.align([a, b, c], start=14)[0]] == [14, 15]
    assert [k for k, _ in S.align([a, b, c], length=2)[0]] == [10, 11]
    assert S.align([a, b, c], start=40)[0] == []


def test_align_by_index():
    a, c = meta([10, 11, 12, 13]), meta([None, 11, 11, 13, 15])
    frames, skipped = S.align([a, c], by_index=True)
    assert frames == [(0, [0, 0]), (1, [1, 1]), (2, [2, 2]), (3, [3, 3]), (4, [None, 4])]
    assert skipped == [{'no_key': 0, 'repeated': 0}] * 2
    assert S.align([a, c], by_index=True, start=1, length=2, min_sources=2)[0] == [(1, [1, 1]), (2, [2, 2])]


# ---- frame_runs ----------------------------------------------------------------------------
def field(istop, valid=True, dropouts=None, linecount=263):
    x = {'valid': valid, 'istop': istop, 'linecount': linecount}
    if dropouts is not None:
        x['dropouts'] = dropouts
    return x


def test_frame_runs_takes_the_last_valid_field_of_each_parity():
    rec = {'fields': [field(True, dropouts=[[5, 1, 2]]),                  # an earlier valid top field: not used
                      field(False, valid=False, dropouts=[[6, 1, 2]]),    # invalid
                      field(False, dropouts=[[30, 100, 120], [31, 0, 910]], linecount=262),
                      field(True, dropouts=[[40, 7, 9]])]}
    runs, counts, nrows, keyed = S.frame_runs(rec, 'NTSC')
    assert nrows == (263, 262) and keyed
    assert counts.sum() == 3 and counts[0, 40] == 1 and counts[1, 30] == 1 and counts[1, 31] == 1
    assert tuple(runs[0, 40, 0]) == (7, 9) and tuple(runs[1, 31, 0]) == (0, 910)
    assert S.frame_runs({'fields': [field(True), field(False, valid=False)]}, 'NTSC') is None
    assert S.frame_runs({'fields': [field(False)]}, 'NTSC') is None
    runs, counts, nrows, keyed = S.frame_runs({'fields': [field(True), field(False, dropouts=[])]}, 'PAL')
    assert not keyed and counts.sum() == 0


def test_frame_runs_caps_a_row_at_eight():
    d = [[50, 10 * k, 10 * k + 5] for k in range(11)]
    runs, counts, _, _ = S.frame_runs({'fields': [field(True, dropouts=d), field(False, dropouts=[])]}, 'PAL')
    assert counts[0, 50] == 8
    assert [tuple(x) for x in runs[0, 50]] == [(10 * k, 10 * k + 5) for k in range(7)] + [(70, 105)]


@pytest.mark.parametrize('bad', [[320, 1, 2], [-1, 1, 2], [5, -1, 2], [5, 4, 4], [5, 9, 3], [5, 900, 911]])
def test_frame_runs_refuses_an_invalid_run(bad):
    rec = {'fields': [field(True, dropouts=[[5, 1, 2], bad]), field(False, dropouts=[])]}
    with pytest.raises(S.StackError, match='src frame 7'):
        S.frame_runs(rec, 'NTSC', 'src frame 7: ')


# ---- residual ------------------------------------------------------------------------------
def random_runs(rng, n_src, W, rows, dense=False):
    runs = np.zeros((n_src, 2, S.MAX_LINES, 8, 2), dtype=np.int16)
    counts = np.zeros((n_src, 2, S.MAX_LINES), dtype=np.int32)
    for s in range(n_src):
        for p in range(2):
            for r in rows:
                n = int(rng.integers(1 if dense else 0, 9))
                for k in range(n):
                    a = int(rng.integers(0, W - 1))
                    runs[s, p, r, k] = (a, min(W, a + int(rng.integers(1, W // (2 if dense else 4)))))
                counts[s, p, r] = n
    return runs, counts


@pytest.mark.parametrize('n_src', [1, 2, 3, 5])
def test_residual_equals_the_per_pixel_and(n_src):
    rng = np.random.default_rng(100 + n_src)
    W, rows = 910, [0, 1, 17, 262, 319]
    runs, counts = random_runs(rng, n_src, W, rows, dense=True)
    res_r, res_c = S.residual(runs, counts, W)
    hit = 0
    for p in range(2):
        for r in range(S.MAX_LINES):
            want = np.ones(W, dtype=bool)
            for s in range(n_src):
                m = np.zeros(W, dtype=bool)
                for k in range(counts[s, p, r]):
                    m[runs[s, p, r, k, 0]:runs[s, p, r, k, 1]] = True
                want &= m
            got = np.zeros(W, dtype=bool)
            iv = [tuple(int(v) for v in res_r[p, r, k]) for k in range(res_c[p, r])]
            for a, b in iv:
                assert 0 <= a < b <= W and not got[a:b].any()
                got[a:b] = True
            assert all(iv[k][1] < iv[k + 1][0] for k in range(len(iv) - 1))     # ascending, merged
            if res_c[p, r] < 8:
                assert np.array_equal(got, want), (p, r)
            hit += int(want.any())
    assert hit >= 4
    # and it is the restatement's residual mask
    H = 525
    frames = np.zeros((n_src, 1, H, W), dtype=np.uint16)
    _, resid = R.stack(frames, np.ones((1, n_src), bool), runs[None], counts[None], 'NTSC', [('median', 0)])
    got = R.run_mask(res_r, res_c, H, W)
    if (res_c < 8).all():
        assert np.array_equal(got, resid[0])


def test_residual_caps_a_row_at_eight():
    runs = np.zeros((2, 2, S.MAX_LINES, 8, 2), dtype=np.int16)
    counts = np.zeros((2, 2, S.MAX_LINES), dtype=np.int32)
    runs[0, 1, 9, 0] = (0, 1135)                                          # one whole row ...
    counts[0, 1, 9] = 1
    for k in range(8):                                                    # ... against eight runs, two of them split
        runs[1, 1, 9, k] = (100 * k, 100 * k + 50)
    counts[1, 1, 9] = 8
    res_r, res_c = S.residual(runs, counts, 1135)
    assert res_c[1, 9] == 8 and res_c.sum() == 8
    assert [tuple(x) for x in res_r[1, 9]] == [(100 * k, 100 * k + 50) for k in range(8)]
    # source 0 in two pieces with a gap inside run 3: nine intersections, the ninth extends the eighth
    runs[0, 1, 9, 0] = (0, 320)
    runs[0, 1, 9, 1] = (330, 1135)
    counts[0, 1, 9] = 2
    res_r, res_c = S.residual(runs, counts, 1135)
    want = [(0, 50), (100, 150), (200, 250), (300, 320), (330, 350), (400, 450), (500, 550), (600, 750)]
    assert res_c[1, 9] == 8 and [tuple(x) for x in res_r[1, 9]] == want
    assert S.runs_list(res_r, res_c, 1)[:2] == [[9, 0, 50], [9, 100, 150]] and S.runs_list(res_r, res_c, 0) == []


# ---- the command's refusals (all before a context is created) ---------------------------------
def run_cli(*args):
    return subprocess.run([sys.executable, CLI, *map(str, args)], capture_output=True, text=True, timeout=120)


def write_source(path, nframes, system='NTSC', nrec=None, extra=0):
    n = R.OUTW[system] * R.FRAME_LINES[system] * 2 * nframes + extra
    with open(str(path) + '.tbc', 'wb') as fh:
        fh.truncate(n)
    with open(str(path) + '.json', 'w') as fh:
        json.dump(meta([None] * (nframes if nrec is None else nrec)), fh)


def refused(r, out, word, reports=0):
    """Non-zero, one line of error (after `reports` lines on frames left out), nothing written."""
    assert r.returncode not in (0, None) and r.returncode > 0, (r.returncode, r.stderr)
    lines = [x for x in r.stderr.splitlines() if x.strip()]
    assert len(lines) == 1 + reports and word in lines[-1], r.stderr
    assert all('left out' in x for x in lines[:-1])
    assert not os.path.exists(str(out) + '.tbc') and not os.path.exists(str(out) + '.json')
    assert not os.path.exists(str(out) + '.tbc.tmp')


def test_cli_refusals(tmp_path):
    out = tmp_path / 'out'
    a = tmp_path / 'a'
    write_source(a, 2)
    refused(run_cli('-o', out), out, 'sources')
    refused(run_cli('-o', out, *[a] * 17), out, 'sources')
    refused(run_cli('-o', out, a, tmp_path / 'nothere'), out, 'no such file')
    os.unlink(str(a) + '.json')
    refused(run_cli('-o', out, a), out, 'no such file')
    write_source(a, 2, extra=2)
    refused(run_cli('-o', out, a), out, 'whole number')
    write_source(a, 2)
    refused(run_cli('-p', '-o', out, a), out, 'whole number')             # NTSC frames read as PAL
    write_source(a, 2, nrec=3)
    refused(run_cli('-o', out, a), out, 'records')
    write_source(a, 2)                                                     # no frame has a frame number
    refused(run_cli('-o', out, a), out, 'no output frame', reports=1)
    refused(run_cli('--by-index', '--start', 5, '-o', out, a), out, 'no output frame')
    assert '.pcm is not stacked' in run_cli('--help').stdout


# ---- the library -----------------------------------------------------------------------------
def test_library_exports_the_stacker():
    from ldgpu import native
    lib = native.load()
    out = subprocess.run(['nm', '-D', '--defined-only', native.LIB_PATH], capture_output=True, text=True).stdout
    for name in ('ldg_stack_frames', 'ldg_conceal_frames'):
        assert name in native.EXPORTS and hasattr(lib, name) and ('T ' + name) in out
    assert lib.ldg_stack_frames(None, 1, 1, None, None, None, None, 2, 3840, None) == -1
    assert lib.ldg_conceal_frames(None, 1, None, None, None, None) == -1
    assert native.STACK_MODES == {m: i for i, m in enumerate(S.MODES)} and native.STACK_MAX_SOURCES == S.MAX_SOURCES
