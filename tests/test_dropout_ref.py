"""The build-defined dropout rules on the CPU: the numpy restatement
(tests/dropout_ref.py) on the oracle's decode of clean captures and of the shared capture
with synthesised dropouts, closed-form known answers of every step of the rule, and the
header's structs against their ctypes mirrors.  The GPU is held to the same restatement
in test_dropout_gpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dropout_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CLEAN_CASES = ['ntsc_cav_u8_mtf0_0p3s', 'pal_cav_u8_mtf_0p3s', 'ntsc_cav_u8_wowbig_0p2s', 'pal_clv_u8_jit_0p3s']


@pytest.mark.parametrize('case', CLEAN_CASES)
def test_clean_captures_have_no_runs(case):
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden
    from oracle.capture import FMT_U8
    from oracle.framer import decode_capture
    system = make_golden.CASES[case]['system']
    seen = []

    def on_field(f):
        if f.valid:
            seen.append(R.detect_field(f.data[0]['demod'], f.linelocs, f.linecount, system))

    decode_capture(make_golden.build_capture(case), FMT_U8, system=system, on_field=on_field)
    assert len(seen) >= 4
    assert all(runs == [] for runs in seen), [runs for runs in seen if runs]


def group_delay(dec):
    """The demod's constant group delay in samples, from the oracle's own demod of the
    capture: how far the centre of the flagged extent of each long dropout lies past the
    centre of the samples that were replaced."""
    d = [((first + last) - (2 * (d0 - f['origin']) + dn - 1)) / 2
         for f in dec['fields'] if f['valid'] for d0, dn, first, last in f['extents']]
    assert len(d) >= 2
    assert max(d) - min(d) < 40, d
    return float(np.mean(d))


def expected_rows(f, delay, system):
    """{row: [(x0, x1)]}: the pixel interval of each synthesised dropout on each row of
    valid field f it covers (shifted by the demod's delay), and the set of those rows."""
    W = R.OUTW[system]
    ll = f['linelocs']
    out = {}
    for d0, dn in R.capture_dropouts(system):
        a, b = d0 - f['origin'] + delay, d0 + dn - f['origin'] + delay        # demod indices [a, b)
        for r in range(f['linecount']):
            begin, end = ll[r + R.LOFF[system]], ll[r + R.LOFF[system] + 1]
            lo, hi = max(a, begin), min(b, end)
            if hi - lo >= 1:
                sc = W / (end - begin)
                out.setdefault(r, []).append(((lo - begin) * sc, (hi - begin) * sc))
    return out


@pytest.mark.parametrize('system', ['NTSC', 'PAL'])
def test_every_dropout_found_and_no_stray_runs(system):
    dec = R.oracle_decode(system)
    assert [f['valid'] for f in dec['fields']] == [False] + [True] * (len(dec['fields']) - 1)
    delay = group_delay(dec)
    print('%s: group delay %.1f samples' % (system, delay))
    assert 100 < delay < 180
    covered = 0
    for f in dec['fields'][1:]:
        want = expected_rows(f, delay, system)
        by_row = {}
        for r, sx, ex in f['runs']:
            by_row.setdefault(r, []).append((sx, ex))
        for r, ivs in want.items():
            for x0, x1 in ivs:
                covered += 1
                assert any(sx < x1 and x0 < ex for sx, ex in by_row.get(r, [])), (f['readsample'], r, x0, x1, by_row.get(r))
        for r in by_row:
            assert any(abs(r - w) <= 1 for w in want), (f['readsample'], r, by_row[r])
        for r, runs in by_row.items():          # the rule's own invariants
            assert len(runs) <= R.MAX_PER_LINE
            assert all(0 <= sx < ex <= R.OUTW[system] for sx, ex in runs)
            assert all(runs[k][1] < runs[k + 1][0] for k in range(len(runs) - 1))
    # all 15 dropouts lie in valid fields; the 6000-sample one spans four rows
    assert covered >= 15 + 3


def test_capture_reaches_the_cap_and_the_fallback():
    """The shared capture exercises what the GPU tests rely on: some row holds
    LDG_MAX_DROPOUTS_PER_LINE runs (its ninth absorbed), and some run's first candidate
    r - d has a run over the same pixels, so it is concealed from r + d."""
    most, fallback = 0, 0
    for system in ('NTSC', 'PAL'):
        dec = R.oracle_decode(system)
        by_read = {f['readsample']: f for f in dec['fields']}
        d = R.LINE_STEP[system]
        for frame, m in zip(dec['frames'], dec['meta']):
            fl = [by_read[x['readsample']] for x in m['fields'] if x['valid']]
            top = next(f for f in fl if f['istop'])
            bot = next(f for f in fl if not f['istop'])
            for f in (top, bot):
                rows = [r for r, _, _ in f['runs']]
                most = max([most] + [rows.count(r) for r in set(rows)])
            _, log = R.conceal_frame(frame, top['runs'], bot['runs'], top['linecount'], bot['linecount'], system)
            fallback += sum(1 for p, r, sx, ex, c in log if c == r + d)
    assert most == R.MAX_PER_LINE
    assert fallback >= 1


# ---- closed-form known answers ------------------------------------------------------------
def flags(n, *idx):
    f = np.zeros(n, dtype=bool)
    f[list(idx)] = True
    return f


def test_merge_gap_80_versus_81():
    ib, ie = 1000, 3000
    one = R.sample_runs(flags(2000, 500, 501, 502, 582, 583, 584), ib, ie)
    assert one == [(1500 - 24, 1584 + 24)]
    # 81 apart: two raw runs (their pads do not touch: 1502 + 24 + 1 < 1583 - 24)
    two = R.sample_runs(flags(2000, 500, 501, 502, 583, 584, 585), ib, ie)
    assert two == [(1476, 1526), (1559, 1609)]
    # two raw runs whose pads touch (1502 + 40 + 1 == 1583 - 40) become one padded run
    assert R.sample_runs(flags(2000, 500, 501, 502, 583, 584, 585), ib, ie, merge_gap=80, pad=40) == [(1460, 1625)]
    assert R.sample_runs(flags(2000, 500, 501, 502, 583, 584, 585), ib, ie, merge_gap=80, pad=39) == \
        [(1461, 1541), (1544, 1624)]


def test_min_flagged_2_versus_3():
    assert R.sample_runs(flags(2000, 500, 580), 0, 2000) == []
    assert R.sample_runs(flags(2000, 500, 540, 580), 0, 2000) == [(476, 604)]
    # the count is of flagged samples, not of the run's length
    assert R.sample_runs(flags(2000, 500, 580), 0, 2000, min_flagged=2) == [(476, 604)]


def test_pad_is_clipped_at_the_row_ends():
    assert R.sample_runs(flags(100, 3, 4, 5, 95, 96, 97), 700, 800, merge_gap=10) == [(700, 729), (771, 799)]


def test_pixels_floor_and_ceil():
    # 2000 samples onto 1000 pixels from begin = 100.5: sample s -> (s - 100.5) / 2
    assert R.pixel_runs([(101, 104)], 100.5, 2100.5, 1000) == [(0, 3)]           # 0.25 .. 2.25
    assert R.pixel_runs([(100, 100)], 100.5, 2100.5, 1000) == [(0, 1)]           # -0.25 clipped to 0
    assert R.pixel_runs([(2090, 2099)], 100.5, 2100.5, 1000) == [(994, 1000)]    # 994.75 .. 999.75
    # touching pixel runs merge (startx <= previous endx), a pixel apart they do not
    assert R.pixel_runs([(200, 209), (211, 220)], 100.0, 2100.0, 1000) == [(50, 61)]
    assert R.pixel_runs([(200, 209), (213, 220)], 100.0, 2100.0, 1000) == [(50, 55), (56, 61)]


def test_ninth_run_is_absorbed():
    runs = [(100 * k, 100 * k + 9) for k in range(11)]
    got = R.pixel_runs(runs, 0.0, 2000.0, 2000)
    assert len(got) == 8
    assert got[:7] == [(100 * k, 100 * k + 10) for k in range(7)]
    assert got[7] == (700, 1010)


def test_detect_row_flags_nan_and_both_sides():
    d = np.full(3000, 8.0e6)
    d[1200:1205] = np.nan
    d[1700:1703] = 1.0e6
    d[2200:2203] = 2.0e7
    d[2600:2602] = 2.0e7                       # two samples only: dropped
    got = R.detect_row(d, 1000.0, 3000.0, 1000, 7.0e6, 1.0e7)
    assert got == [(88, 115), (338, 364), (588, 614)]


def frame_of(system, seed=5):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 60000, size=(R.FRAME_LINES[system], R.OUTW[system]), dtype=np.uint16)


def test_conceal_order_and_overlap_fallback():
    fr = frame_of('NTSC')
    # row 100 of the top field: r - d = 98 is clean -> from 98
    out, log = R.conceal_frame(fr, [(100, 50, 60)], [], 263, 262, 'NTSC')
    assert log == [(0, 100, 50, 60, 98)]
    assert np.array_equal(out[200, 50:60], fr[196, 50:60])
    changed = out != fr
    assert changed[200, 50:60].any() and changed.sum() == changed[200, 50:60].sum()
    # 98 has a run over the range -> r + d; 98 and 102 -> r - 2d; all four -> left alone
    runs = [(98, 55, 70), (100, 50, 60)]
    out, log = R.conceal_frame(fr, runs, [], 263, 262, 'NTSC')
    assert (0, 100, 50, 60, 102) in log and np.array_equal(out[200, 50:60], fr[204, 50:60])
    # (row 98's own run [55, 70) takes 96: row 100's run overlaps it)
    assert (0, 98, 55, 70, 96) in log
    runs = [(98, 55, 70), (100, 50, 60), (102, 59, 61)]
    out, log = R.conceal_frame(fr, runs, [], 263, 262, 'NTSC')
    assert (0, 100, 50, 60, 96) in log and np.array_equal(out[200, 50:60], fr[192, 50:60])
    runs = [(96, 0, 910), (98, 55, 70), (100, 50, 60), (102, 59, 61), (104, 10, 51)]
    out, log = R.conceal_frame(fr, runs, [], 263, 262, 'NTSC')
    assert (0, 100, 50, 60, None) in log and np.array_equal(out[200], fr[200])
    # a run that only touches the range does not block a candidate
    out, log = R.conceal_frame(fr, [(98, 60, 70), (100, 50, 60)], [], 263, 262, 'NTSC')
    assert (0, 100, 50, 60, 98) in log
    # the bottom field's rows are the odd frame rows; PAL steps by 4
    frp = frame_of('PAL')
    out, log = R.conceal_frame(frp, [], [(100, 0, 30)], 313, 312, 'PAL')
    assert log == [(1, 100, 0, 30, 96)] and np.array_equal(out[201, :30], frp[193, :30])


def test_conceal_keeps_flag_pixels_vbi_rows_and_the_frame_end():
    fr = frame_of('NTSC')
    out, _ = R.conceal_frame(fr, [(100, 0, 10)], [], 263, 262, 'NTSC')
    assert np.array_equal(out[200, :2], fr[200, :2]) and np.array_equal(out[200, 2:10], fr[196, 2:10])
    # rows below LDG_CONCEAL_FIRST_ROW are not written ...
    out, log = R.conceal_frame(fr, [(20, 100, 200), (10, 0, 910)], [(20, 5, 9)], 263, 262, 'NTSC')
    assert log == [] and np.array_equal(out, fr)
    # ... and not read: row 21's r - d = 19 is out, it takes r + d = 23; row 22 takes 24 (20 is out)
    out, log = R.conceal_frame(fr, [(21, 100, 200), (22, 100, 200)], [], 263, 262, 'NTSC')
    assert log == [(0, 21, 100, 200, 23), (0, 22, 100, 200, 24)]
    # PAL: first row 22, no flag pixels
    frp = frame_of('PAL')
    out, log = R.conceal_frame(frp, [(21, 0, 9), (22, 0, 9)], [], 312, 313, 'PAL')
    assert log == [(0, 22, 0, 9, 26)] and np.array_equal(out[44, :9], frp[52, :9])
    # sources stay inside the frame's picture rows: 2 * min(lt, lb)
    out, log = R.conceal_frame(fr, [(261, 30, 40), (262, 30, 40)], [], 263, 262, 'NTSC')
    assert log == [(0, 261, 30, 40, 259)]


def test_abi_struct_sizes(tmp_path):
    """ctypes mirrors == the C compiler's view of include/ldgpu.h, and the header's constants."""
    from ldgpu import native
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ldgpu.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(ldg_dropout_opts), '
                   'offsetof(ldg_dropout_opts, merge_gap), offsetof(ldg_dropout_opts, conceal), sizeof(ldg_dropout), '
                   'offsetof(ldg_dropout, endx), LDG_MAX_DROPOUTS_PER_LINE, LDG_CONCEAL_FIRST_ROW(LDG_SYSTEM_NTSC), '
                   'LDG_CONCEAL_FIRST_ROW(LDG_SYSTEM_PAL));return 0;}')
    exe = tmp_path / 'sz'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    O, D = native.DropoutOpts, native.Dropout
    assert got == [ctypes.sizeof(O), O.merge_gap.offset, O.conceal.offset, ctypes.sizeof(D), D.endx.offset,
                   native.MAX_DROPOUTS_PER_LINE, R.FIRST_ROW['NTSC'], R.FIRST_ROW['PAL']]
    assert ctypes.sizeof(O) == 32 and ctypes.sizeof(D) == 8 and R.MAX_PER_LINE == native.MAX_DROPOUTS_PER_LINE
    for f in ('ldg_dropout_defaults', 'ldg_set_dropout_opts', 'ldg_field_dropouts'):
        assert f in native.EXPORTS


def test_defaults_match_the_library():
    from ldgpu import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip('libldgpu.so not built')
    for system in ('NTSC', 'PAL'):
        assert native.dropout_defaults(system) == R.defaults(system)
    lib = native.load()
    assert lib.ldg_dropout_defaults(2, ctypes.byref(native.DropoutOpts())) == -1
    assert lib.ldg_set_dropout_opts(None, None) == -1


def test_cli_flags_and_cut_rejection(tmp_path):
    """The CLI lists the flags, and -c (cut) rejects them before any device is opened."""
    cli = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
    r = subprocess.run([sys.executable, cli, '-h'], capture_output=True, text=True, timeout=120)
    for opt in ('--dropouts', '--conceal', '--dropout-lo-ire', '--dropout-hi-ire'):
        assert opt in r.stdout
    for flags in (['--dropouts'], ['--conceal'], ['--dropout-hi-ire', '120']):
        r = subprocess.run([sys.executable, cli, '-c', *flags, str(tmp_path / 'x.u8'), str(tmp_path / 'out')],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'ERROR: --dropouts / --conceal apply to a decode' in r.stdout
