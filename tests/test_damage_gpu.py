"""The field kernels on captures with damaged sync pulses (tests/damage.py), stage by stage
against the oracle's Field of the same read, and the whole decode of captures that carry
several damages against the oracle's decode loop.

The rest of the suite holds csrc/field.hip and the failure exits of csrc/tbc.hip to the oracle
only where every peak-walk chain joins, every hsync is regular and both vsync votes are
non-zero.  Here the peak list, the vsync rows and their vote repair, the status code of every
way out of Field.__init__, nextfieldoffset, the reprinted log lines, the filled and
extrapolated line locations and linebad are compared on reads built to leave that path
(test_damage_ref.py asserts on the CPU that they do).  The bars are DESIGN.md "Parity"'s: sync
analysis and metadata exact, line locations within 1e-6 samples, .tbc within +-1 LSB, .pcm
within +-1; none is loosened for damaged lines.
"""
import numpy as np
import pytest

import damage as D

pytestmark = pytest.mark.gpu


def _status(outcome):
    from ldgpu import native
    return {'valid': native.FS_VALID, 'no_vsync': native.FS_NO_VSYNC, 'short': native.FS_SHORT,
            'linelocs': native.FS_LINELOCS, 'tbc': native.FS_TBC, 'crash': native.FS_CRASH}[outcome]


def _log_flags(lines):
    """ldg_field_info.log_flags rebuilt from what the oracle printed."""
    from ldgpu import native
    fl = 0
    for l in lines:
        if l.startswith('vsync vote needed'):
            fl |= 1 << int(l.split()[-1])
        elif l == D.NOVS:
            fl |= native.LOG_NO_VSYNC
    return fl


def check_read(case, expect, r, inf, ctx, slot):
    """One decoded read (ldg_field_info `inf`, debug arrays of `slot`) against the oracle's Read `r`
    of the same samples."""
    from ldgpu import native
    ntsc = r.system == 'NTSC'
    W = 910 if ntsc else 1135
    f, start = r.field, r.start
    assert r.outcome == expect['outcome']         # (test_damage_ref.py / test_vbi_ref.py: the capture does its job)
    assert inf.status == _status(r.outcome), (start, r.outcome, inf.status)
    peaks = r.crash_peaks if f is None else f.peaklist
    assert inf.npeaks == len(peaks), start
    assert np.array_equal(ctx.debug(slot, 41, np.int32, inf.npeaks), np.asarray(peaks)), start
    if f is None:
        print('%s read %d: crash' % (case, start))
        return
    assert inf.nvsync == len(f.vsyncs), start
    for q in range(inf.nvsync):
        assert list(inf.vsync[q]) == [int(x) for x in f.vsyncs[q]], (start, q)
    assert inf.nextfieldoffset == f.nextfieldoffset, start
    if len(peaks) >= 200:
        assert abs(inf.med_hsync - f.med_hsync) <= 1e-12 * abs(f.med_hsync), start
        assert abs(inf.hsync_tol - f.hsync_tolerance) <= 1e-12 * abs(f.hsync_tolerance), start
    assert inf.log_flags == _log_flags(r.log), (start, r.log, inf.log_flags)
    if not f.valid:
        print('%s read %d: %s, %d peaks, %d vsyncs' % (case, start, r.outcome, inf.npeaks, inf.nvsync))
        return
    assert inf.istop == int(f.istop) and inf.linecount == f.linecount, start
    for j, l in enumerate(r.rf.SysParams['philips_codelines']):
        lc = f.linecode[l]
        assert bool(inf.linecode_ok[j]) == (lc is not None), (start, l)
        if lc is not None:
            assert list(inf.linecode[j]) == [int(x) for x in lc], (start, l)
    for k, got in (('minutes', inf.vbi_minutes), ('seconds', inf.vbi_seconds), ('clvframe', inf.vbi_clvframe),
                   ('framenr', inf.vbi_framenr), ('status', inf.vbi_status)):
        assert (None if got == native.VBI_NONE else int(got)) == f.vbi[k], (start, k)
    assert bool(inf.vbi_isclv) == bool(f.vbi['isclv'])
    nl = f.linecount + 4
    stages = [(20, f.linelocs1), (21, f.linelocs2), (24, f.linelocs)]
    if ntsc:
        stages += [(22, f.linelocs3), (23, f.linelocs4)]
    for what, arr in stages:
        arr = np.asarray(arr, dtype=np.float64)
        assert arr.size == nl
        err = np.abs(ctx.debug(slot, what, np.float64, nl) - arr).max()
        assert err < 1e-6, (start, what, err)
    bad = np.asarray(f.linebad, dtype=bool)
    assert np.array_equal(ctx.debug(slot, 31, np.uint8, nl).astype(bool), bad), start
    if ntsc:
        assert np.array_equal(ctx.debug(slot, 30, np.float32, nl), f.burstlevel), start
    pic = ctx.debug(slot, 40, np.uint16, f.linecount * W)
    assert pic.size == f.dspicture.size
    d = np.abs(pic.astype(np.int64) - f.dspicture.astype(np.int64))
    assert d.max() <= 1, (start, d.max())
    pcm, counts, nxt = ctx.field_audio([slot], [0.0])
    assert counts[0] * 2 == f.dsaudio.size
    da = np.abs(pcm[0, :2 * counts[0]].astype(np.int64) - f.dsaudio.astype(np.int64))
    assert da.max() <= 1, (start, da.max())
    assert nxt[0] == f.audio_next_offset
    print('%s read %d: valid, %d bad lines, .tbc %d of %d samples off by 1, .pcm %d of %d' % (
        case, start, int(bad.sum()), int((d != 0).sum()), d.size, int((da != 0).sum()), da.size))


@pytest.mark.parametrize('case', list(D.CASES))
def test_stage_parity(case, gpu_ctx_ntsc, gpu_ctx_pal):
    """Every read of the case: status, peaks, vsyncs, nextfieldoffset, hsync median, log flags;
    on valid fields also the VBI, every line-location stage, linebad, burst levels, the
    resampled picture and the audio.  One test per case: the contexts are session-wide, so
    every debug array is read here, right after the decode."""
    c = D.CASES[case]
    ntsc = c['system'] == 'NTSC'
    data = D.capture(case)
    ctx, _ = gpu_ctx_ntsc if ntsc else gpu_ctx_pal
    ctx.set_capture(data, data.size, 0, 0)
    assert len(c['reads']) <= 8
    infos = ctx.decode_reads(c['reads'], [1.0] * len(c['reads']))
    for slot in range(len(c['reads'])):
        check_read(case, c['expect'][slot], D.oracle_read(case, slot), infos[slot], ctx, slot)


def _decode(dec):
    got = []
    dec.decode(sink=lambda fr, au, meta: got.append((fr.copy(), au.copy(), meta)))
    return got


def _same_frames(name, got, o):
    """Frames, audio and metadata of a decode against the oracle's; the off-by-one counts."""
    import json
    off = total = pcm_off = pcm_all = 0
    for (fr, au, m), f, a, want in zip(got, o['frames'], o['pcm'], o['meta']):
        assert json.loads(json.dumps(m)) == json.loads(json.dumps(want))
        assert fr.size == f.size
        d = np.abs(fr.astype(np.int64) - f.astype(np.int64))
        assert d.max() <= 1
        off, total = off + int((d != 0).sum()), total + d.size
        assert au.size == a.size
        da = np.abs(au.astype(np.int64) - a.astype(np.int64))
        assert da.max() <= 1
        pcm_off, pcm_all = pcm_off + int((da != 0).sum()), pcm_all + da.size
    return '%s: %d frames, .tbc %d of %d samples off by 1, .pcm %d of %d' % (name, len(got), off, total, pcm_off, pcm_all)


@pytest.mark.parametrize('name', ['ntsc_cav', 'ntsc_clv', 'pal_cav'])
@pytest.mark.parametrize('batch', [3, 16])
def test_end_to_end_vs_oracle(name, batch):
    """The whole decode (planner, speculative launches, replay) of a capture whose fields include
    `short` reads, a `tbc` failure and a three-vsync field whose nextfieldoffset lands mid-field,
    against the oracle's decode loop: the same frames, metadata (the `fields` lists with their
    invalid reads and MTF levels) exact, .tbc within +-1 LSB, .pcm within +-1.  (No `no_vsync` field here:
    it sends the reference one second on, past the end of a capture this short, where its demod raises;
    test_reference_crash_mid_decode has one.)"""
    from ldgpu.decoder import GPUDecoder
    from oracle.capture import FMT_U8
    w, o = D.WHOLE[name], D.oracle_whole(name)
    assert not o['crashed'] and len(o['frames']) >= 3
    seen = {f['outcome'] for f in o['fields']}
    if any(f['outcome'] == 'valid' and f['nvsync'] >= 3 and f['nextfieldoffset'] < 400000 for f in o['fields']):
        seen.add('three_vs')
    assert seen >= w['want'] | {'short'}, seen
    dec = GPUDecoder(system=w['system'], batch=batch)
    dec.set_capture(o['data'], FMT_U8)
    got = _decode(dec)
    st = dec.stats
    dec.ctx.close()
    assert len(got) == len(o['frames'])
    print(_same_frames(name, got, o) + '; batch=%d: reads %d, used %d' % (batch, st['reads'], st['reads_used']))


@pytest.mark.parametrize('batch', [3, 16])
def test_reference_crash_mid_decode(batch):
    """A capture on which the oracle's decode loop raises ReferenceCrash after two frames (a
    `no_vsync` field sends it one second on, to a read with a vsync within its first 11 peaks):
    GPUDecoder.decode raises its ReferenceCrash too, after handing its sink the same frames."""
    from ldgpu.decoder import GPUDecoder, ReferenceCrash
    from oracle.capture import FMT_U8
    w, o = D.WHOLE['ntsc_crash'], D.oracle_whole('ntsc_crash')
    assert o['crashed'] and 'first 11 peaks' in o['crashed'] and len(o['frames']) >= 2
    dec = GPUDecoder(system=w['system'], batch=batch)
    dec.set_capture(o['data'], FMT_U8)
    got = []
    with pytest.raises(ReferenceCrash):
        dec.decode(sink=lambda fr, au, meta: got.append((fr.copy(), au.copy(), meta)))
    dec.ctx.close()
    assert len(got) == len(o['frames'])
    print(_same_frames('ntsc_crash', got, o))
