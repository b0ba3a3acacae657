"""The oracle reproduces its committed golden fixtures, and decodes the synthetic
captures to the frame numbers / CLV time codes the generator wrote."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle.capture import FMT_BY_EXT
from oracle.framer import decode_capture

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')


def load_case(case):
    import sys
    sys.path.insert(0, GOLD)
    import make_golden
    with open(os.path.join(GOLD, case + '.json')) as fh:
        return make_golden, json.load(fh)


# captures with time-base error (make_golden.py): disc speed 1 + a1 sin + a2 sin
WOW_CASES = ['ntsc_cav_u8_wow_0p2s', 'pal_clv_u8_wow_0p25s', 'ntsc_cav_lds_wow_0p15s']
WOWBIG_CASES = ['ntsc_cav_u8_wowbig_0p2s', 'pal_cav_u8_wowbig_0p25s']
JIT_CASES = ['ntsc_cav_u8_jit_0p3s', 'pal_clv_u8_jit_0p3s']
_TIMEBASE = {}           # case -> what the decode below saw of the oracle's own line locations


def oracle_run(case):
    """The oracle's decode of a golden case, and (kept per case for the time-base checks
    below) each valid field's final line locations, its linelocs2 and the frames' ends."""
    mg, gold = load_case(case)
    data = mg.build_capture(case)
    c = mg.CASES[case]
    fields = []

    def on_field(f):
        if f.valid:
            fields.append((np.array(f.linelocs, dtype=np.float64), np.array(f.linelocs2, dtype=np.float64)))
    frames, pcm, meta = decode_capture(data, FMT_BY_EXT[c['fmt']], system=c['system'], on_field=on_field)
    _TIMEBASE[case] = (fields, [m['nextsample'] for m in meta])
    return mg, gold, data, frames, pcm, meta


def timebase(case):
    if case not in _TIMEBASE:
        oracle_run(case)
    return _TIMEBASE[case]


@pytest.mark.parametrize('case', ['ntsc_cav_u8_0p2s', 'ntsc_clv_u8_0p2s', 'ntsc_cav_r30_0p15s', 'ntsc_cav_lds_0p15s',
                                  'pal_clv_u8_0p2s', 'pal_clv_lds_0p15s',
                                  'ntsc_cav_s16_0p15s', 'ntsc_cav_u8_mid_0p2s'] + WOW_CASES + WOWBIG_CASES + JIT_CASES)
def test_oracle_matches_golden(case):
    mg, gold, data, frames, pcm, meta = oracle_run(case)
    assert hashlib.sha256(data).hexdigest() == gold['capture_sha256']
    assert len(frames) == len(gold['frames'])
    for f, a, m, g in zip(frames, pcm, meta, gold['frames']):
        assert hashlib.sha256(f.tobytes()).hexdigest() == g['tbc_sha256']
        assert hashlib.sha256(a.tobytes()).hexdigest() == g['pcm_sha256']
        assert m == g['meta']
    if frames and 'comb_rgb48_sha256' in gold['frames'][0]:
        from oracle.comb import Comb2D
        rgb = Comb2D().process(np.stack(frames))
        assert [hashlib.sha256(r.tobytes()).hexdigest() for r in rgb] == \
            [g['comb_rgb48_sha256'] for g in gold['frames']]


def test_synthetic_vbi_frame_numbers():
    _, gold = load_case('ntsc_cav_u8_0p2s')
    nrs = [g['meta']['vbi']['framenr'] for g in gold['frames']]
    assert nrs == list(range(nrs[0], nrs[0] + len(nrs)))
    _, gold = load_case('ntsc_clv_u8_0p2s')
    nrs = [g['meta']['vbi']['framenr'] for g in gold['frames']]
    assert nrs == [5400, 5401, 5402, 5403]
    assert all(g['meta']['vbi']['isclv'] for g in gold['frames'])


# ---- time-base error: the captures are what they claim (a later change to the synth cannot
# ---- silently turn them back into rigid ones) ------------------------------------------------

def test_wow_capture_does_not_depend_on_its_chunks():
    """The disc time is closed-form in the sample index, the noise is drawn per fixed block and
    the FM phase is one running sum: 0.05 s generated in chunks of 2^20, of 2^22 and of
    300,007 samples (no multiple of anything) is the same capture, byte for byte."""
    from ldgpu.synth import make_capture
    mg, _ = load_case('ntsc_cav_u8_wowbig_0p2s')
    n = int(40e6 * 0.05)
    for case in ('ntsc_cav_u8_wowbig_0p2s', 'pal_clv_u8_wow_0p25s'):
        c = mg.CASES[case]
        a = make_capture(n, 'u8', chunk=1 << 20, system=c['system'], **c['kw'])
        b = make_capture(n, 'u8', chunk=1 << 22, system=c['system'], **c['kw'])
        assert a == b
        assert a == make_capture(n, 'u8', chunk=300007, system=c['system'], **c['kw'])
        rigid = make_capture(n, 'u8', system=c['system'], **{k: v for k, v in c['kw'].items() if k != 'wow'})
        assert a != rigid


def line_spans(case):
    """Integer spans int(ll[l + 1]) - int(ll[l]) of the final line locations, over the valid
    fields of the oracle's decode: what sets ldg_k_final_lines' rows-per-thread split."""
    fields, _ = timebase(case)
    assert len(fields) >= 4
    return np.concatenate([np.diff(ll.astype(np.int64)) for ll, _ in fields])


@pytest.mark.parametrize('case,least', [(c, 14) for c in WOW_CASES] + [(c, 40) for c in WOWBIG_CASES])
def test_wow_line_spans_leave_the_fixed_point(case, least):
    """A rigid capture's lines span 2541..2543 (NTSC) / 2559..2561 (PAL) samples.  Measured
    here: 2533..2552 and 2517..2568 NTSC, 2551..2570 and 2534..2588 PAL."""
    sp = line_spans(case)
    print(case, 'line spans', sp.min(), '..', sp.max())
    assert sp.max() - sp.min() >= least
    assert sp.max() < 2816               # SPL_MAXN (csrc/tbc.hip): still the whole-line solve


@pytest.mark.parametrize('case', WOWBIG_CASES)
def test_wowbig_head_gaps_are_replaced(case):
    """refine_linelocs_hsync's head repair (lddecode_core.py:772-777) replaces a gap outside
    linelen +- 0.2 us by linelen itself: some field has at least 5 of its first ten linelocs2
    gaps equal to rf.linelen (a measured gap never is)."""
    from oracle.demod import RFDemod
    mg, _ = load_case(case)
    linelen = RFDemod(system=mg.CASES[case]['system']).linelen
    fields, _ = timebase(case)
    replaced = [int((np.abs(np.diff(ll2)[:10] - linelen) < 1e-6).sum()) for _, ll2 in fields]
    print(case, 'replaced head gaps per field', replaced)
    assert max(replaced) >= 5


def frame_length_errors(case):
    """(frame lengths nextsample[k + 1] - nextsample[k] minus the nominal 40e6 / fps samples,
    the planner's probe half-window int(0.3 * linelen))."""
    from oracle.demod import RFDemod
    mg, _ = load_case(case)
    rf = RFDemod(system=mg.CASES[case]['system'])
    _, ends = timebase(case)
    assert len(ends) >= 4
    return np.diff(np.array(ends, dtype=np.float64)) - rf.freq_hz / rf.SysParams['FPS'], int(0.3 * rf.linelen)


@pytest.mark.parametrize('case', JIT_CASES)
def test_jit_frame_lengths_are_probe_territory(case):
    """Every frame is off nominal by more than the sample or two a rigid capture's sync peaks
    jitter by, and by less than the probe half-window: a predicted start misses, its probe
    finds the field.  Measured: -18.7..18.3 NTSC, -11..23 PAL."""
    err, halfwin = frame_length_errors(case)
    print(case, 'frame length - nominal', err)
    assert (np.abs(err) > 2).all() and (np.abs(err) < halfwin).all()


@pytest.mark.parametrize('case', WOWBIG_CASES)
def test_wowbig_frame_lengths_pass_the_probe_window(case):
    """Some frame is off nominal by more than the probe half-window (762 / 768 samples): a
    predicted start is then wrong by more than a probe can mend.  Measured: -795 NTSC, 864 PAL."""
    err, halfwin = frame_length_errors(case)
    print(case, 'frame length - nominal', err)
    assert np.abs(err).max() > halfwin
