"""The row kernels' outputs bit for bit.  tests/golden/rows_bits.json holds
SHA-256 hashes of what the burst, hsync and final-resample kernels and the default 2D comb leave
behind, written on an MI355X by the commit the fixture's header names.  A change to those
kernels that is meant to be exact (instruction counts, lane assignment, divisions by constants)
must reproduce every hash; the hashes are regenerated only when arithmetic is changed on purpose:

    python tests/test_rows_bits_gpu.py COMMIT        (LDGPU_LIB: the library of that commit)

Per field read: the record's status and, for a valid field, its linecount, the line locations
after each stage (debug 21 - 24: linelocs2, 3, 4 and the final ones; PAL has 2 and the final
ones), burstlevel (NTSC) and the field picture.  Per NTSC case: the default 2D comb's rgb48 of
three frames woven from the case's field pictures and the burst-level state carried out, with
the FilterIQ chunks' warm-up (the default) and with LDG_COMB_IQW=0 (the one-lane fallback).

Cases: an NTSC and a PAL golden capture (ldg_k_final_lines and tbc_pixel serve both), a
time-base case whose lines are far enough off nominal that the rows-per-thread split of the
final pass changes, and a damaged-sync case with a line of several nominal lengths (the
windowed solves of the burst and final passes)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'rows_bits.json')
# (case, where its capture comes from)
CASES = [('ntsc_cav_u8_0p2s', 'golden'), ('pal_clv_lds_0p15s', 'golden'), ('ntsc_cav_u8_wowbig_0p2s', 'golden'),
         ('first_half', 'damage')]
NREADS = 4
SPL_MAXN = 2816                 # csrc/tbc.hip: lines of this many samples or more are solved in windows
LONG_CASE, WOW_CASE = 'first_half', 'ntsc_cav_u8_wowbig_0p2s'
NFRAMES = 3


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _capture(case, src):
    """(system, capture bytes / array, sample format, n samples, read starts or None for the chain from 0)."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    from ldgpu.formats import NAME_TO_FMT, samples_in_bytes
    if src == 'damage':
        import damage
        c = damage.CASES[case]
        data = damage.capture(case)
        return c['system'], data, 0, data.size, list(c['reads'])
    import make_golden
    with open(os.path.join(HERE, 'golden', case + '.json')) as fh:
        gold = json.load(fh)
    data = make_golden.build_capture(case)
    assert hashlib.sha256(data).hexdigest() == gold['capture_sha256']
    fmt = NAME_TO_FMT[gold['settings']['fmt']]
    return gold['settings']['system'], data, fmt, samples_in_bytes(fmt, len(data)), None


def _weave(pics, W):
    """NFRAMES frames of 525 x W from the field pictures in turn (rows cropped / zero-padded)."""
    fr = np.zeros((NFRAMES, 525, W), dtype=np.uint16)
    for k in range(2 * NFRAMES):
        p = pics[k % len(pics)].reshape(-1, W)
        rows = fr[k // 2, (k & 1)::2]
        n = min(rows.shape[0], p.shape[0])
        rows[:n] = p[:n]
    return fr


def _comb(native, rf, frames, iqw):
    old = os.environ.pop('LDG_COMB_IQW', None)
    if iqw is not None:
        os.environ['LDG_COMB_IQW'] = iqw
    try:
        ctx = native.Context('NTSC', 0, max_reads=2)
        try:
            ctx.set_filters(rf.params(), rf.tables)
            ctx.comb_reset()
            rgb = ctx.comb_ntsc(frames)
            return {'rgb48': [_sha(x) for x in rgb], 'state': _sha(ctx.debug(0, 51, np.float64, 1))}
        finally:
            ctx.close()
    finally:
        os.environ.pop('LDG_COMB_IQW', None)
        if old is not None:
            os.environ['LDG_COMB_IQW'] = old


def case_hashes(case, src):
    """{'reads': [per read {what: sha256 / int}], 'comb': {...}, 'comb_iqw0': {...}} on the GPU."""
    from ldgpu import native
    from ldgpu.rfparams import RFTables
    system, data, fmt, nsamp, starts = _capture(case, src)
    ntsc = system == 'NTSC'
    W = 910 if ntsc else 1135
    rf = RFTables(system)
    ctx = native.Context(system, 0, max_reads=2)
    reads, pics = [], []
    try:
        ctx.set_filters(rf.params(), rf.tables)
        ctx.set_capture(data, nsamp, fmt, 0)
        s, k = (0 if starts is None else starts[0]), 0
        while k < (NREADS if starts is None else len(starts)):
            inf = ctx.decode_reads([s], [1.0])[0]
            assert inf.status not in (native.FS_EOF, native.FS_MIGRATED, native.FS_PENDING), (case, s, inf.status)
            h = {'start': int(s), 'status': int(inf.status)}
            if inf.status == 0:
                # (a field that is not valid has no line count: its record keeps whatever was there)
                h['linecount'] = int(inf.linecount)
                nl = int(inf.linecount) + 4
                for what in ((21, 22, 23, 24) if ntsc else (21, 24)):
                    a = ctx.debug(0, what, np.float64, nl)
                    assert a.size == nl
                    h[str(what)] = _sha(a)
                    sp = np.diff(a.astype(np.int64))
                    h['span%d' % what] = [int(sp.min()), int(sp.max())]
                if ntsc:
                    h['30'] = _sha(ctx.debug(0, 30, np.float32, nl))
                pic = ctx.debug(0, 40, np.uint16, int(inf.linecount) * W)
                assert pic.size == int(inf.linecount) * W
                h['40'] = _sha(pic)
                pics.append(pic.copy())
            reads.append(h)
            k += 1
            if starts is None:
                s += int(inf.nextfieldoffset)
            elif k < len(starts):
                s = starts[k]
    finally:
        ctx.close()
    out = {'reads': reads}
    if ntsc:
        assert pics, case
        frames = _weave(pics, W)
        out['comb'] = _comb(native, rf, frames, None)
        out['comb_iqw0'] = _comb(native, rf, frames, '0')
    return out


def _differences(got, want, where=''):
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), where
        return [d for k in sorted(want) for d in _differences(got[k], want[k], where + '/' + str(k))]
    if isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        return [d for i, (g, w) in enumerate(zip(got, want)) for d in _differences(g, w, where + '/%d' % i)]
    return [] if got == want else [where]


def _count(x):
    return sum(_count(v) for v in (x.values() if isinstance(x, dict) else x)) if isinstance(x, (dict, list)) else 1


def _covered(case, h):
    """The paths the case is here for were taken (a fixture on the main path hides a failure)."""
    valid = [r for r in h['reads'] if r['status'] == 0]
    assert valid, case
    if case == LONG_CASE:
        # a line of SPL_MAXN samples or more: the windowed solves (burst pass: linelocs2, final pass: the last ones)
        assert max(r['span21'][1] for r in valid) >= SPL_MAXN
        assert max(r['span24'][1] for r in valid) >= SPL_MAXN
    if case == WOW_CASE:
        # the final pass gives a thread 11 rows of a line's n - 3: lines 40 samples apart end three threads
        # apart, so the thread that holds the partial chunk moves (it stays in the line's last wave)
        assert max(r['span24'][1] for r in valid) - min(r['span24'][0] for r in valid) >= 40
    if 'comb' in h:
        assert len(h['comb']['rgb48']) == len(h['comb_iqw0']['rgb48']) == NFRAMES
        # the fallback chain gives the same picture (tests/test_comb.py), so it was compared, not skipped
        assert h['comb'] == h['comb_iqw0']
        assert len(set(h['comb']['rgb48'])) > 1


@pytest.fixture(scope='module')
def fixture_hashes():
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    assert fx['header']['commit'] and 'regenerated only' in fx['header']['note']
    return fx['hashes']


@pytest.mark.gpu
@pytest.mark.parametrize('case,src', CASES)
def test_rows_outputs_bit_for_bit(case, src, fixture_hashes):
    got = case_hashes(case, src)
    want = fixture_hashes[case]
    bad = _differences(got, want, case)
    print('%s: %d values compared, %d differ' % (case, _count(want), len(bad)))
    assert not bad, bad
    _covered(case, got)


def test_fixture_is_whole():
    """(no GPU) Every case and read has its hashes, and the long-line, time-base and fallback
    paths are in them."""
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    assert sorted(fx['hashes']) == sorted(c for c, _ in CASES)
    for case, _ in CASES:
        h = fx['hashes'][case]
        ntsc = not case.startswith('pal')
        assert len(h['reads']) >= 1
        for r in h['reads']:
            assert {'start', 'status'} <= set(r)
            if r['status'] == 0:
                keys = {'21', '24', '40'} | ({'22', '23', '30'} if ntsc else set())
                assert keys | {'linecount'} <= set(r)
                assert all(len(r[k]) == 64 for k in keys)
            else:
                assert set(r) == {'start', 'status'}
        assert ('comb' in h) == ntsc and ('comb_iqw0' in h) == ntsc
        _covered(case, h)


if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'ld-decode_amd'), HERE]
    note = ('SHA-256 of the row kernels\' outputs per field read and of the default 2D comb '
            '(tests/test_rows_bits_gpu.py). Written on an MI355X by the library of the commit named here; '
            'regenerated only when the row kernels\' arithmetic is changed on purpose.')
    fx = {'header': {'commit': sys.argv[1], 'note': note, 'nreads': NREADS},
          'hashes': {case: case_hashes(case, src) for case, src in CASES}}
    dst = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, 'w') as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', dst)
