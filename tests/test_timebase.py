"""The decode on captures with time-base error (wow and flutter).

Every other capture of the suite comes from a rigid clock: each line is 2542 +- 1 (NTSC) or
2560 +- 1 (PAL) samples, each frame its nominal length to a sample or two.  The cases here
(tests/golden/make_golden.py, SynthRF's ``wow``) vary the disc's speed, so that

  * the line spans cover ~19 (``wow``) to ~54 (``wowbig``) samples: ldg_k_final_lines' rows per
    thread, its linspace step and the wow factor leave their fixed point, and in ``wowbig``
    refine_linelocs_hsync's head / tail repair replaces gaps outside linelen +- 0.2 us;
  * the frames are tens (``jit``) to hundreds (``wow``, ``wowbig``) of samples off nominal: the
    planner's predicted read starts miss by less, and by more, than a start probe can mend.

test_oracle_golden.py checks on the CPU that the captures have these properties.  Here the
HIP path is held to the oracle on them with the bars of DESIGN.md "Parity": demod channels
within 1e-9 relative, audio channels within 1e-3 Hz, peak lists, vsyncs, nextfieldoffset and
all per-field metadata exact, line locations within 1e-6 samples, .tbc within +-1 LSB, .pcm
within +-1.
"""
import json
import os
import sys

import numpy as np
import pytest

from test_gpu_parity import oracle_decode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

STAGE_CASES = ['ntsc_cav_u8_wow_0p2s', 'ntsc_cav_u8_wowbig_0p2s', 'pal_clv_u8_wow_0p25s', 'pal_cav_u8_wowbig_0p25s']
ALL_CASES = STAGE_CASES + ['ntsc_cav_u8_jit_0p3s', 'pal_clv_u8_jit_0p3s', 'ntsc_cav_lds_wow_0p15s']
JIT_CASES = ['ntsc_cav_u8_jit_0p3s', 'pal_clv_u8_jit_0p3s']
PROBE_CASES = JIT_CASES + ['ntsc_cav_u8_wowbig_0p2s', 'pal_cav_u8_wowbig_0p25s']
NREADS = 4


@pytest.mark.parametrize('case', STAGE_CASES)
def test_stage_parity(case, gpu_ctx_ntsc, gpu_ctx_pal):
    """The first four reads of the oracle's own chain from sample 0 (s += nextfieldoffset),
    every stage against the oracle's Field of the same read.  One test per case: the
    contexts are session-wide and other modules reuse their slots, so every debug array is
    read here, right after the decode."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden
    from ldgpu import native
    from oracle.capture import FMT_U8, Capture
    from oracle.demod import RFDemod
    from oracle.field import FieldNTSC, FieldPAL
    system = make_golden.CASES[case]['system']
    ntsc = system == 'NTSC'
    data = make_golden.build_capture(case)
    orf = RFDemod(system=system)
    cap = Capture(data, FMT_U8)
    ref, s = [], 0
    for _ in range(NREADS):
        raw = orf.demod(cap, s, 1000000, 1.0)
        f = (FieldNTSC if ntsc else FieldPAL)(orf, raw, 0, audio_offset=0)
        ref.append((s, raw, f))
        s += int(f.nextfieldoffset)
    ctx, _ = gpu_ctx_ntsc if ntsc else gpu_ctx_pal
    buf = np.frombuffer(data, np.uint8)
    ctx.set_capture(buf, buf.size, 0, 0)
    infos = ctx.decode_reads([r[0] for r in ref], [1.0] * NREADS)
    W = 910 if ntsc else 1135
    nvalid, spans, replaced = 0, [], 0
    for slot, (start, raw, f) in enumerate(ref):
        inf = infos[slot]
        # demod
        for ci, ch in enumerate(['demod', 'demod_05', 'demod_sync', 'demod_burst'] + ([] if ntsc else ['demod_pilot'])):
            o = raw[0][ch]
            g = ctx.debug(slot, ci, np.float64, o.size)
            assert g.size == o.size
            err = np.abs(g - o).max() / max(np.abs(o).max(), 1.0)
            assert err < 1e-9, (start, ch, err)
        for ci, ch in enumerate(['audio_left', 'audio_right']):
            o = raw[1][ch]
            g = ctx.debug(slot, 10 + ci, np.float64, o.size)
            assert g.size == o.size
            assert np.abs(g - o).max() < 1e-3, (start, ch)
        # sync analysis
        assert inf.npeaks == len(f.peaklist)
        assert np.array_equal(ctx.debug(slot, 41, np.int32, inf.npeaks), np.asarray(f.peaklist))
        assert inf.nvsync == len(f.vsyncs)
        for q in range(inf.nvsync):
            assert list(inf.vsync[q]) == [int(x) for x in f.vsyncs[q]]
        assert inf.nextfieldoffset == f.nextfieldoffset
        assert (inf.status == 0) == bool(f.valid), (start, inf.status)
        if not f.valid:
            continue
        nvalid += 1
        assert inf.istop == int(f.istop) and inf.linecount == f.linecount
        for k, got in (('minutes', inf.vbi_minutes), ('seconds', inf.vbi_seconds), ('clvframe', inf.vbi_clvframe),
                       ('framenr', inf.vbi_framenr), ('status', inf.vbi_status)):
            assert (None if got == native.VBI_NONE else int(got)) == f.vbi[k], (start, k)
        assert bool(inf.vbi_isclv) == bool(f.vbi['isclv'])
        # line locations
        nl = f.linecount + 4
        stages = [(20, f.linelocs1), (21, f.linelocs2), (24, f.linelocs)]
        if ntsc:
            stages += [(22, f.linelocs3), (23, f.linelocs4)]
        for what, arr in stages:
            arr = np.asarray(arr, dtype=np.float64)
            assert arr.size == nl
            g = ctx.debug(slot, what, np.float64, nl)
            err = np.abs(g - arr).max()
            assert err < 1e-6, (start, what, err)
        assert np.array_equal(ctx.debug(slot, 31, np.uint8, nl).astype(bool), np.asarray(f.linebad, dtype=bool)), start
        if ntsc:
            assert np.array_equal(ctx.debug(slot, 30, np.float32, nl), f.burstlevel)
        # resampled picture and audio
        pic = ctx.debug(slot, 40, np.uint16, f.linecount * W)
        assert pic.size == f.dspicture.size
        d = np.abs(pic.astype(np.int64) - f.dspicture.astype(np.int64))
        assert d.max() <= 1, (start, d.max())
        pcm, counts, nxt = ctx.field_audio([slot], [0.0])
        assert counts[0] * 2 == f.dsaudio.size
        da = np.abs(pcm[0, :2 * counts[0]].astype(np.int64) - f.dsaudio.astype(np.int64))
        assert da.max() <= 1, (start, da.max())
        assert nxt[0] == f.audio_next_offset
        print('%s read %d: .tbc %d of %d samples off by 1, .pcm %d of %d' % (
            case, start, int((d != 0).sum()), d.size, int((da != 0).sum()), da.size))
        spans.append(np.diff(np.asarray(f.linelocs).astype(np.int64)))
        replaced = max(replaced, int((np.abs(np.diff(np.asarray(f.linelocs2))[:10] - orf.linelen) < 1e-6).sum()))
    # not vacuous: these reads see the time-base error (and, in wowbig, the head repair at work)
    assert nvalid >= 3
    spans = np.concatenate(spans)
    assert spans.max() - spans.min() >= (40 if 'wowbig' in case else 14), (spans.min(), spans.max())
    if 'wowbig' in case:
        assert replaced >= 5


def _decode(dec):
    got = []
    dec.decode(sink=lambda fr, au, meta: got.append((fr.copy(), au.copy(), meta)))
    return got


@pytest.mark.parametrize('case', ALL_CASES)
@pytest.mark.parametrize('batch', [3, 16])
def test_end_to_end_vs_oracle(case, batch):
    """The whole decode (planner, speculative launches, replay) against the oracle's decode of
    the same capture, itself pinned to the committed fixture: the same frames, metadata and
    read chain exact, .tbc within +-1 LSB, .pcm within +-1."""
    from ldgpu.decoder import GPUDecoder
    from ldgpu.formats import NAME_TO_FMT
    data, gold, frames, pcm, meta = oracle_decode(case)
    c = gold['settings']
    dec = GPUDecoder(system=c['system'], batch=batch)
    dec.set_capture(data, NAME_TO_FMT[c['fmt']])
    got = _decode(dec)
    st = dec.stats
    dec.ctx.close()
    assert len(got) == len(gold['frames']) >= 2
    exact = pcm_same = pcm_all = 0
    for (fr, au, m), f, a, g in zip(got, frames, pcm, gold['frames']):
        assert m == g['meta']
        assert fr.size == f.size
        d = np.abs(fr.astype(np.int64) - f.astype(np.int64))
        assert d.max() <= 1
        exact += int((d == 0).all())
        assert au.size == g['pcm_len'] == a.size
        da = np.abs(au.astype(np.int64) - a.astype(np.int64))
        assert da.max() <= 1
        pcm_same += int((da == 0).sum())
        pcm_all += da.size
    print('%s batch=%d: %d/%d frames bit-identical, %d/%d .pcm samples identical; reads %d, used %d, '
          'jitter misses %d, probes %d, moved %d' % (
              case, batch, exact, len(got), pcm_same, pcm_all, st['reads'], st['reads_used'],
              st.get('jitter_misses', 0), st.get('probes', 0), st.get('probe_moved', 0)))


@pytest.mark.parametrize('case', PROBE_CASES)
def test_probe_modes_give_the_same_decode(case, monkeypatch):
    """LDG_PROBE 0, 1 and unset (PAL: on; NTSC: on after jitter misses) on frames tens of
    samples off nominal (jit: inside the probe window) and hundreds (wowbig: outside it):
    the probes choose where speculative reads start, never what the decode outputs."""
    from ldgpu.decoder import GPUDecoder
    from ldgpu.formats import NAME_TO_FMT
    data, gold, frames, pcm, meta = oracle_decode(case)
    c = gold['settings']
    outs, stats = [], []
    for mode in ('0', '1', None):
        if mode is None:
            monkeypatch.delenv('LDG_PROBE', raising=False)
        else:
            monkeypatch.setenv('LDG_PROBE', mode)
        dec = GPUDecoder(system=c['system'], batch=16)
        dec.set_capture(data, NAME_TO_FMT[c['fmt']])
        outs.append(_decode(dec))
        stats.append(dec.stats)
        dec.ctx.close()
        st = dec.stats
        print('%s LDG_PROBE=%s: reads %d, used %d (%.2f per read used), jitter misses %d, probes %d, moved %d' % (
            case, mode, st['reads'], st['reads_used'], st['reads'] / max(st['reads_used'], 1),
            st.get('jitter_misses', 0), st.get('probes', 0), st.get('probe_moved', 0)))
    assert stats[0].get('probes', 0) == 0
    if case in JIT_CASES:
        assert stats[1].get('probe_moved', 0) > 0       # else the case says nothing about probes
    assert len(outs[0]) == len(gold['frames'])
    assert [m for _, _, m in outs[0]] == [g['meta'] for g in gold['frames']]
    for other in outs[1:]:
        assert len(other) == len(outs[0])
        for (f0, a0, m0), (f1, a1, m1) in zip(outs[0], other):
            assert np.array_equal(f0, f1)
            assert np.array_equal(a0, a1)
            assert json.dumps(m0, sort_keys=True, default=str) == json.dumps(m1, sort_keys=True, default=str)
