"""What the video cut trims besides the video channels: demod_05, the
audio carrier slices and audio phase 1 of the tail blocks, audio phase 2's last block.
The decode must not change by a bit, and a field that would read trimmed data must come
back FS_VCUT (decoded again in full) before the replay accepts it."""
import os
import sys

import numpy as np
import pytest

from test_gpu_parity import oracle_decode

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NTSC_CUT = 740000

# stats['vcut_redo'] of the commit before the trimming (the video cut alone), batch 8, default cut,
# measured on an MI355X with that commit's library: the trimming's guards must add none
PARENT_REDO = {'ntsc_clv_u8_0p2s': 0, 'ntsc_cav_u8_mid_0p2s': 8, 'pal_clv_u8_0p2s': 0}


def _decode(dec, **kw):
    got = []
    dec.decode(sink=lambda fr, au, m: got.append((fr.copy(), au.copy(), m)), **kw)
    return got


def _same(a, b):
    assert len(a) == len(b) and len(a) > 0
    for (f0, a0, m0), (f1, a1, m1) in zip(a, b):
        assert m0 == m1
        assert np.array_equal(f0, f1)
        assert np.array_equal(a0, a1)


@pytest.mark.parametrize('case', ['ntsc_clv_u8_0p2s', 'ntsc_cav_u8_mid_0p2s', 'pal_clv_u8_0p2s'])
def test_default_cut_gives_the_uncut_decode(case, monkeypatch):
    """No cut against the default cut: frames, .pcm and metadata bit for bit, and no read
    redone that the video cut alone did not redo.  PAL's cut trims no audio at all."""
    from ldgpu import native
    from ldgpu.decoder import GPUDecoder
    from ldgpu.formats import NAME_TO_FMT
    data, gold, frames, pcm, meta = oracle_decode(case)
    c = gold['settings']
    outs, redos = [], []
    for cut in ('0', None):
        if cut is None:
            monkeypatch.delenv('LDG_VCUT', raising=False)
        else:
            monkeypatch.setenv('LDG_VCUT', cut)
        dec = GPUDecoder(system=c['system'], batch=8)
        dec.set_capture(data, NAME_TO_FMT[c['fmt']])
        outs.append(_decode(dec))
        redos.append(dec.stats.get('vcut_redo', 0))
        plan = native.tail_plan(1001026, 62565, 15641, dec.video_cut)
        dec.ctx.close()
    print('%s: vcut_redo %r (parent %d), plan %r' % (case, redos, PARENT_REDO[case], plan))
    _same(outs[0], outs[1])
    assert redos[0] == 0 and redos[1] == PARENT_REDO[case]
    if c['system'] == 'PAL':
        assert plan[:4] == (None, None, 4, 66)          # every audio block stays
    else:
        assert plan[:4] == (48640, 11609, 3, 51)


def test_one_read_with_and_without_the_cut():
    """One steady-state read through the context, cut and uncut, in the same slot: demod_05
    below the cut, audio-2 below acut2, the line locations, the peaks and the record are equal
    bit for bit (what lies past them is not written with the cut, and nothing reads it)."""
    from ldgpu import native
    from ldgpu.rfparams import RFTables
    data, gold, *_ = oracle_decode('ntsc_clv_u8_0p2s')
    start, mtf = gold['stage']['readsample'], gold['stage']['mtf_level']
    assert start > 1024
    rf = RFTables('NTSC')
    ctx = native.Context('NTSC', 0, max_reads=2)
    try:
        ctx.set_filters(rf.params(), rf.tables)
        buf = np.frombuffer(data, np.uint8)
        ctx.set_capture(buf, buf.size, 0, 0)
        acut1, acut2 = native.tail_plan(1001026, 62565, 15641, NTSC_CUT)[:2]
        got = []
        for cut in (NTSC_CUT, 0):
            ctx.set_video_cut(cut)
            info = ctx.decode_reads([start], [mtf])[0]
            assert info.status == native.FS_VALID
            got.append(dict(rec=bytes(info),
                            d05=ctx.debug(0, 1, np.float64, 1001026)[:NTSC_CUT].copy(),
                            a2=[ctx.debug(0, 10 + ch, np.float64, 15641)[:acut2].copy() for ch in (0, 1)],
                            a1=[ctx.debug(0, 12 + ch, np.float64, 62565)[:acut1].copy() for ch in (0, 1)],
                            lines=[ctx.debug(0, w, np.float64, 320).copy() for w in (20, 21, 22, 23, 24)],
                            peaks=ctx.debug(0, 41, np.int32, 2048).copy(),
                            pcm=[x.copy() for x in ctx.field_audio([0], [0.0])]))
        a, b = got
        assert a['d05'].size == NTSC_CUT and a['a2'][0].size == acut2
        assert a['rec'] == b['rec']
        assert np.array_equal(a['d05'], b['d05'])
        for k in ('a2', 'a1', 'lines', 'pcm'):
            for x, y in zip(a[k], b[k]):
                assert np.array_equal(x, y, equal_nan=True), k
        assert np.array_equal(a['peaks'], b['peaks'])
    finally:
        ctx.close()


SWEEP_CASE = 'ntsc_cav_u8_mid_0p2s'
QUARTERS = 12                      # a quarter line apart: three line lengths
MARGIN = 100                       # samples: the prediction below is from the oracle's final locations


def _sweep_plan():
    """The sweep's start offsets, and for each what the oracle's line locations of the first
    field say about its guards: (start, video guards fire, the trimming's guards fire), or None
    where a guard's bound lies within MARGIN of the cut.  The first field's locations move
    rigidly with the start (the same field, the same samples)."""
    import json
    from test_tail_trim_host import golden_field
    rf, lines, lc = golden_field(SWEEP_CASE)
    with open(os.path.join(HERE, 'golden', SWEEP_CASE + '.json')) as fh:
        r0 = json.load(fh)['stage']['readsample']
    lines = lines + (r0 - 1024 if r0 > 1024 else 0)        # positions in the capture
    q = rf.linelen / 4.0
    # at `base` the last video window ends a quarter line above the cut, so the sweep walks
    # down from "video" through "trimming only" to "none"
    base = int(lines[lc + 1] + 1 - NTSC_CUT - q) + 1024
    plan = []
    for k in range(QUARTERS):
        s = base + int(round(k * q))
        ll = lines - (s - 1024)                            # positions in the read that starts at s (> 1024)
        video = ll[lc + 1] + 1          # ldg_k_final_lines' last window (the burst and VBI windows end sooner)
        trim = ll[lc + 3] + 400 + 3 * 40 + 2    # ldg_k_hsync_lines' bound on the last of linecount + 4 lines
        audio = max(ll[lc + 1], ll[lc + 2])     # ldg_audio_reach
        if min(abs(video - NTSC_CUT), abs(trim - NTSC_CUT)) < MARGIN:
            plan.append((s, None, None))
        else:
            plan.append((s, bool(video >= NTSC_CUT), bool(trim >= NTSC_CUT or audio >= 64 * 11609)))
    return plan


def test_sweep_has_the_case_it_is_for():
    """(no GPU work) The sweep below holds starts whose first field has every video window
    below the cut and still reaches trimmed data, starts that reach the video cut, and none
    in the first line that reads a negative position."""
    plan = _sweep_plan()
    assert all(s > 1024 for s, _, _ in plan)
    assert sum(1 for _, v, t in plan if v is False and t is True) >= 3
    assert any(v for _, v, _ in plan)


@pytest.fixture(scope='module')
def sweep_decoders(monkeypatch_module):
    from ldgpu.decoder import GPUDecoder
    decs = []
    for cut in ('0', None):
        if cut is None:
            monkeypatch_module.delenv('LDG_VCUT', raising=False)
        else:
            monkeypatch_module.setenv('LDG_VCUT', cut)
        decs.append(GPUDecoder(system='NTSC', batch=1))     # no speculative reads: only the chain's own
    yield decs
    for d in decs:
        d.ctx.close()


@pytest.fixture(scope='module')
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.mark.parametrize('k', range(QUARTERS))
def test_start_sweep_across_the_guards(k, sweep_decoders):
    """The first frame from start offsets a quarter line apart, so that the first field's end
    walks across the cut: every start gives its own uncut decode bit for bit; a start whose
    video windows all lie below the cut but whose line refinement (demod_05 of the field's
    last lines) reaches past it is redone -- the video guards alone would have accepted it
    with trimmed data.  (With regular line spacing the audio guard cannot fire without the
    line-refinement guard: that one covers linecount + 4 lines plus 522 samples against a cut
    at or below 64 acut2, the audio linecount + 2 lines.  Its bound is tested on the CPU,
    tests/test_tail_trim_host.py; here the two are seen as a pair.)  Measured: the eight
    such starts of the sweep are redone once each, the two starts past them not at all."""
    from ldgpu.formats import NAME_TO_FMT
    data, gold, *_ = oracle_decode(SWEEP_CASE)
    s, video, trim = _sweep_plan()[k]
    outs, redo = [], []
    for dec in sweep_decoders:
        dec.set_capture(data, NAME_TO_FMT[gold['settings']['fmt']])
        before = dec.stats.get('vcut_redo', 0)
        outs.append(_decode(dec, start_sample=s, length=1))
        redo.append(dec.stats.get('vcut_redo', 0) - before)
    print('start %d: predicted video %r trimming %r, vcut_redo %r' % (s, video, trim, redo))
    _same(outs[0], outs[1])
    assert redo[0] == 0
    if video is False and trim is True:
        assert redo[1] >= 1
    if video is False and trim is False:
        assert redo[1] == 0                  # the guards do not fire on what the cut leaves whole
