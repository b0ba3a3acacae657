"""Disc stacking on the GPU (csrc/stack.hip) against the numpy restatement of the
build-defined rule (tests/stack_ref.py): ldg_stack_frames exactly equal
to it on packed frames of both systems (the second and third PAL frames start off every
16-byte boundary, as in a file), ldg_conceal_frames exactly dropout_ref.conceal_frame, and
disc_stacker.py end to end on a real decode."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dropout_ref as D
import stack_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DECODE = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
STACKER = os.path.join(ROOT, 'ld-decode_amd', 'disc_stacker.py')
SYSTEMS = ['NTSC', 'PAL']
COMBOS = [(m, T) for m in R.MODES for T in (0, 3840, 65535)]
_ctx = {}


def context(system, max_frames=3):
    """One context per (system, max_frames) for the module; ldg_set_dropout_opts is never called."""
    from ldgpu import native
    if (system, max_frames) not in _ctx:
        _ctx[system, max_frames] = native.Context(system, 0, max_reads=1, max_frames=max_frames)
    return _ctx[system, max_frames]


def teardown_module(module):
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def make_case(system, n_src, n_frames, seed):
    """(frames uint16 [S, F, H, W], present, runs, counts): a seeded per-pixel base plus
    per-source noise of about the default threshold, 0 and 65535 present, the pixels under a
    run overwritten with the far extreme (ignoring a run then changes the answer)."""
    rng = np.random.default_rng(seed)
    W, H = R.OUTW[system], R.FRAME_LINES[system]
    S, F = n_src, n_frames
    base = rng.integers(0, 65536, (F, H, W)).astype(np.int32)
    base[:, 5, 5:7] = (0, 65535)
    frames = np.empty((S, F, H, W), dtype=np.uint16)
    for s in range(S):
        frames[s] = np.clip(base + np.rint(rng.normal(0, 3840, base.shape)).astype(np.int32), 0, 65535)
    frames[:, :, 5, 5] = 0
    frames[:, :, 5, 6] = 65535
    present = np.ones((F, S), dtype=bool)
    if S >= 2:
        present[1, 0] = False                              # an absent source 0: base moves
    if S >= 3:
        present[1, S - 1] = False
    runs = np.zeros((F, S, 2, R.MAX_LINES, 8, 2), dtype=np.int16)
    counts = np.zeros((F, S, 2, R.MAX_LINES), dtype=np.int32)
    last = (H - 1) >> 1                                    # the last frame row: parity 0, this field row
    for f in range(F):
        for s in range(S):
            for p in range(2):
                for r in np.flatnonzero(rng.random(last + 1) < 0.12):
                    n = int(rng.integers(1, 9))
                    a = rng.integers(0, W, n)
                    runs[f, s, p, r, :n, 0] = a
                    runs[f, s, p, r, :n, 1] = np.minimum(W, a + rng.integers(1, 200, n))
                    counts[f, s, p, r] = n

    def put(f, s, p, r, rr, count=None):
        runs[f, s, p, r] = 0
        runs[f, s, p, r, :len(rr)] = rr
        counts[f, s, p, r] = len(rr) if count is None else count

    put(0, 0, 0, 30, [(0, W)])                             # a whole row, startx = 0 and endx = W
    put(0, S - 1, 1, 31, [(1, 2), (2, 3), (W - 1, W)])     # one pixel at x = 1, 2 (meeting) and W - 1
    put(0, 0, 1, 40, [(100, 200), (200, 300)])             # meeting end to start
    put(0, 0, 0, last, [(W - 9, W)])                       # the last frame row
    put(0, 0, 0, 70, [(-5, 4), (W - 3, W + 7)], count=11)  # the device's clamps (step 6)
    for s in range(S):                                     # masked in every source
        put(0, s, 0, 50, [(300, 340)])
        put(F - 1, s, 0, last, [(3, 20)])
        put(1, s, 1, 60, [(0, 5)])                         # ... with absent sources, over the burst flag pixels
        put(0, s, 1, 61, [(0, W)])
    far = np.where(base < 32768, 65535, 0).astype(np.uint16)
    for f in range(F):
        for s in range(S):
            m = R.run_mask(runs[f, s], counts[f, s], H, W)
            frames[s, f][m] = far[f][m]
    return frames, present, runs, counts


def check(system, frames, present, runs, counts, combos, ctx=None):
    ctx = ctx or context(system)
    want, resid = R.stack(frames, present, runs, counts, system, combos)
    bad = []
    for mode, T in combos:
        got = ctx.stack_frames(list(frames), present, runs, counts, mode=mode, threshold=T)
        diff = got != want[mode, T]
        print('%s N=%d %s T=%d: %d of %d pixels differ' % (system, frames.shape[0], mode, T, int(diff.sum()), diff.size))
        if diff.any():
            f, y, x = (int(v[0]) for v in np.nonzero(diff))
            bad.append((mode, T, int(diff.sum()), (f, y, x), int(got[f, y, x]), int(want[mode, T][f, y, x])))
    assert not bad, bad
    return want, resid


@pytest.mark.parametrize('n_src', [1, 2, 3, 4, 7, 8])
@pytest.mark.parametrize('system', SYSTEMS)
def test_stack_equals_restatement(system, n_src):
    frames, present, runs, counts = make_case(system, n_src, 3, 1000 + n_src)
    _, resid = check(system, frames, present, runs, counts, COMBOS)
    assert resid.any() and not resid.all()
    assert frames.min() == 0 and frames.max() == 65535


@pytest.mark.parametrize('system', SYSTEMS)
def test_stack_sixteen_sources(system):
    frames, present, runs, counts = make_case(system, 16, 2, 1016)
    check(system, frames, present, runs, counts, COMBOS)


def test_stack_without_runs_and_with_a_source_present_nowhere():
    frames, present, _, _ = make_case('PAL', 4, 3, 7)
    ctx = context('PAL')
    want, _ = R.stack(frames, present, None, None, 'PAL', COMBOS[-1:])
    got = ctx.stack_frames(list(frames), present, mode='smart-mean', threshold=65535)
    assert np.array_equal(got, want[COMBOS[-1]])
    present[:, 1] = False
    want, _ = R.stack(frames, present, None, None, 'PAL', COMBOS[:1])
    got = ctx.stack_frames([frames[0], None, frames[2], frames[3]], present, mode='median', threshold=0)
    assert np.array_equal(got, want[COMBOS[0]])


def test_stack_in_chunks():
    """5 frames through the binding's chunk loop at max_frames = 2 equal one call at 5."""
    frames, present, runs, counts = make_case('NTSC', 3, 5, 55)
    combo = [('smart-mean', 3840)]
    want, _ = check('NTSC', frames, present, runs, counts, combo, ctx=context('NTSC', 5))
    got = context('NTSC', 2).stack_frames(list(frames), present, runs, counts)
    assert np.array_equal(got, want[combo[0]])


def test_stack_argument_errors():
    from ldgpu import native
    frames, present, runs, counts = make_case('NTSC', 2, 2, 9)
    ctx = context('NTSC')
    lib = ctx.lib
    srcs = [np.ascontiguousarray(frames[s]) for s in range(2)]
    pres = np.ascontiguousarray(present, dtype=np.uint8)
    out = np.zeros(frames.shape[1:], dtype=np.uint16)

    def call(n_src=2, mode=2, threshold=3840, present=pres, ptrs=None):
        p = (C.c_void_p * 17)(*(ptrs if ptrs is not None else [a.ctypes.data for a in srcs]))
        return lib.ldg_stack_frames(ctx.h, 2, n_src, p, present.ctypes.data, runs.ctypes.data, counts.ctypes.data,
                                    mode, threshold, out.ctypes.data)

    none = pres.copy()
    none[1] = 0
    for kw, word in ((dict(n_src=0), 'n_src'), (dict(n_src=17), 'n_src'), (dict(mode=3), 'mode'), (dict(mode=-1), 'mode'),
                     (dict(threshold=-1), 'threshold'), (dict(threshold=65536), 'threshold'),
                     (dict(present=none), 'present'), (dict(ptrs=[srcs[0].ctypes.data, None]), 'src')):
        assert call(**kw) == -1, kw
        msg = lib.ldg_last_error(ctx.h).decode()
        print(kw.keys(), '->', msg)
        assert 'ldg_stack_frames' in msg and word in msg
    with pytest.raises(native.LDGError, match='threshold'):
        ctx.stack_frames(srcs, pres, runs, counts, threshold=70000)
    check('NTSC', frames, present, runs, counts, COMBOS[-1:])             # a valid call afterwards


def random_field_runs(rng, system, linecount):
    """[(row, startx, endx)] in (row, startx) order, at most 8 a row, with neighbours LINE_STEP
    apart over the same pixels (the first candidate row is then refused)."""
    W, d = D.OUTW[system], D.LINE_STEP[system]
    rows = set(int(r) for r in rng.integers(D.FIRST_ROW[system] - 3, linecount + 2, 40))
    rows |= {r + d for r in list(rows)[:8]} | {r - d for r in list(rows)[8:12]}
    out = []
    for r in sorted(x for x in rows if 0 <= x < R.MAX_LINES):
        starts = sorted(int(a) for a in rng.integers(0, W - 1, int(rng.integers(1, 9))))
        for a in starts:
            out.append((r, a, min(W, a + int(rng.integers(1, 300)))))
    return out


@pytest.mark.parametrize('system', SYSTEMS)
def test_conceal_frames_equals_restatement(system):
    rng = np.random.default_rng(77)
    W, H = D.OUTW[system], D.FRAME_LINES[system]
    n = 3
    frames = rng.integers(0, 65536, (n, H, W)).astype(np.uint16)
    full = (H + 1) // 2
    nrows = np.array([(full, full - 1), (full - 1, full), (full, full)], dtype=np.int32)
    runs = np.zeros((n, 2, R.MAX_LINES, 8, 2), dtype=np.int16)
    counts = np.zeros((n, 2, R.MAX_LINES), dtype=np.int32)
    lists = []
    for f in range(n):
        both = [random_field_runs(rng, system, int(nrows[f, p])) for p in range(2)]
        if f == 0:
            both[0] += [(100, 0, W), (100 + D.LINE_STEP[system], 0, 5)]       # from x = 0: the burst flag pixels stay
        for p in range(2):
            both[p].sort()
            for r, sx, ex in both[p]:
                runs[f, p, r, counts[f, p, r]] = (sx, ex)
                counts[f, p, r] += 1
        lists.append(both)
    assert counts.max() <= 8
    got = context(system, 2).conceal_frames(frames, runs, counts, nrows)      # 3 frames, 2 a call
    changed = 0
    for f in range(n):
        want, log = D.conceal_frame(frames[f], lists[f][0], lists[f][1], int(nrows[f, 0]), int(nrows[f, 1]), system)
        diff = int((got[f] != want).sum())
        print('%s frame %d: %d runs, %d pixels differ' % (system, f, len(log), diff))
        assert diff == 0
        changed += int((want != frames[f]).sum())
        assert any(c is not None and c != r - D.LINE_STEP[system] for _, r, _, _, c in log)
    assert changed > 0


# ---- end to end on a real decode ---------------------------------------------------------------
def run(cmd, *args):
    r = subprocess.run([sys.executable, cmd, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


@pytest.fixture(scope='module', params=SYSTEMS)
def decoded(request, tmp_path_factory):
    """dropout_ref.capture(system) through lddecode.py: `a` with --dropouts, `ac` with --conceal."""
    system = request.param
    d = tmp_path_factory.mktemp('stack_' + system)
    cap = d / 'cap.u8'
    cap.write_bytes(bytes(D.capture(system)))
    flag = ['-p'] if system == 'PAL' else []
    run(DECODE, *flag, '--dropouts', cap, d / 'a')
    run(DECODE, *flag, '--conceal', cap, d / 'ac')
    W, H = D.OUTW[system], D.FRAME_LINES[system]
    tbc = np.fromfile(str(d / 'a.tbc'), dtype=np.uint16).reshape(-1, H, W)
    meta = json.load(open(d / 'a.json'))
    assert len(tbc) == len(meta) >= 4
    return system, d, flag, tbc, meta


def used_fields(rec):
    valid = [x for x in rec['fields'] if x['valid']]
    return [x for x in valid if x['istop']][-1], [x for x in valid if not x['istop']][-1]


def test_cli_stacking_a_source_with_itself(decoded):
    system, d, flag, tbc, meta = decoded
    assert sum(len(x['dropouts']) for m in meta for x in used_fields(m)) >= 10
    for mode in R.MODES:
        run(STACKER, *flag, '--mode', mode, '-o', d / ('aaa_' + mode), d / 'a', d / 'a', d / 'a')
        assert (d / ('aaa_' + mode + '.tbc')).read_bytes() == (d / 'a.tbc').read_bytes()
        out = json.load(open(d / ('aaa_' + mode + '.json')))
        assert len(out) == len(meta)
        for i, (o, m) in enumerate(zip(out, meta)):
            assert o['frame'] == i and o['stack'] == {'framenr': m['vbi']['framenr'], 'sources': [0, 1, 2]}
            assert o['vbi'] == m['vbi'] and len(o['fields']) == 2
            assert [x['dropouts'] for x in used_fields(o)] == [x['dropouts'] for x in used_fields(m)]


def test_cli_second_source_fills_the_dropouts(decoded):
    system, d, flag, tbc, meta = decoded
    rng = np.random.default_rng(3)
    b = np.clip(tbc.astype(np.int32) + rng.integers(-900, 901, tbc.shape), 0, 65535).astype(np.uint16)
    b.tofile(str(d / 'b.tbc'))
    with open(d / 'b.json', 'w') as fh:
        json.dump([dict(m, fields=[{k: v for k, v in x.items() if k != 'dropouts'} for x in m['fields']]) for m in meta], fh)
    r = run(STACKER, *flag, '-o', d / 'ab', d / 'a', d / 'b')
    assert r.stderr.count("without 'dropouts'") == 1 and 'b.json' in r.stderr
    out = np.fromfile(str(d / 'ab.tbc'), dtype=np.uint16).reshape(tbc.shape)
    om = json.load(open(d / 'ab.json'))
    assert all(x['dropouts'] == [] for o in om for x in o['fields'])
    covered = 0
    x0 = 2 if system == 'NTSC' else 0
    for f, m in enumerate(meta):
        for p, x in enumerate(used_fields(m)):
            for row, sx, ex in x['dropouts']:
                y = 2 * row + p
                if y < tbc.shape[1]:
                    assert np.array_equal(out[f, y, max(sx, x0):ex], b[f, y, max(sx, x0):ex]), (f, y, sx, ex)
                    covered += ex - max(sx, x0)
    assert covered > 0
    if system == 'NTSC':
        assert np.array_equal(out[:, :, :2], tbc[:, :, :2])                # base's burst flag pixels
    # elsewhere two candidates 900 apart at the most: their rounded mean
    want = (tbc.astype(np.int32) + b + 1) >> 1
    assert (out.astype(np.int32) == want).mean() > 0.95


def test_cli_conceal_is_the_decode_s_conceal(decoded):
    system, d, flag, tbc, meta = decoded
    run(STACKER, *flag, '--conceal', '-o', d / 'sc', d / 'a')
    assert (d / 'sc.tbc').read_bytes() == (d / 'ac.tbc').read_bytes()
    assert (d / 'ac.tbc').read_bytes() != (d / 'a.tbc').read_bytes()
    # the .json keeps the residual: with one source, its own runs
    out = json.load(open(d / 'sc.json'))
    assert [[x['dropouts'] for x in used_fields(o)] for o in out] == [[x['dropouts'] for x in used_fields(m)] for m in meta]


def test_cli_alignment(decoded):
    """Two sources cut from `a` start two frames apart; their frame numbers still line up."""
    system, d, flag, tbc, meta = decoded
    n = len(meta)
    keys = [m['vbi']['framenr'] for m in meta]
    assert None not in keys and keys == sorted(set(keys)), keys
    for name, lo, hi in (('s1', 0, n - 2), ('s2', 2, n)):
        tbc[lo:hi].tofile(str(d / (name + '.tbc')))
        with open(d / (name + '.json'), 'w') as fh:
            json.dump(meta[lo:hi], fh)
    run(STACKER, *flag, '-o', d / 'al', d / 's1', d / 's2')
    assert (d / 'al.tbc').read_bytes() == (d / 'a.tbc').read_bytes()       # the union's frames
    out = json.load(open(d / 'al.json'))
    assert [o['stack']['framenr'] for o in out] == keys and [o['frame'] for o in out] == list(range(n))
    assert [o['stack']['sources'] for o in out] == [[0]] * 2 + [[0, 1]] * (n - 4) + [[1]] * 2
    run(STACKER, *flag, '--start', keys[2], '--length', 1, '-o', d / 'al1', d / 's1', d / 's2')
    assert (d / 'al1.tbc').read_bytes() == tbc[2].tobytes()
    both = [sys.executable, STACKER, *flag, '--min-sources', '2', '-o', str(d / 'al2'), str(d / 's1'), str(d / 's2')]
    r = subprocess.run(both, capture_output=True, text=True, timeout=600)
    if n > 4:
        assert r.returncode == 0 and (d / 'al2.tbc').read_bytes() == tbc[2:n - 2].tobytes()
    else:                                                  # no frame is in both sources
        assert r.returncode != 0 and 'no output frame' in r.stderr and not (d / 'al2.tbc').exists()
