"""The sync walk's window argmax with 32-bit indices (csrc/field.hip wave_argmax / tile_argmax:
read positions as unsigned 32-bit words, SyncTile::idx's INT64_MAX read as the "no candidate"
word that loses every comparison).  np.argmax order must hold exactly: the first maximum of a
window, every tie to the lower index.

The peaks (debug read 41, as test_gpu_parity.py reads them) are compared with the oracle's
Field.get_syncpeaks in two ways: on a golden read with the oracle's whole decode (peaks and
vsyncs exactly equal; the levels at the peaks and the hsync median within 1e-9 relative, the
bar DESIGN.md "Parity" sets for the demod channels: the FFTs' round-off differs), and, on every
case, with get_syncpeaks run over the GPU's own demod_sync channel (debug read 2), which must
give the GPU's peak list exactly.  Cases: a golden read; a capture of constant samples
(demod_sync is one value throughout: every window ties, no tile has an output above the others,
and no window has a peak); a carrier at the sync-tip frequency (the detector is on throughout, so
demod_sync is a plateau a hair under 1, above the peak threshold: each window's maximum is
decided among nearly equal neighbours and, in most windows, exactly equal ones: the first must win)."""
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NSAMP = 1400000                      # one read of the synthetic captures, with its lead


def _walk(ds, linelen):
    """The oracle's get_syncpeaks over a demod_sync channel."""
    from oracle.field import Field
    f = types.SimpleNamespace(data=[{'demod_sync': ds}], start=0, inlinelen=linelen, rf=types.SimpleNamespace(linelen=linelen))
    return [int(p) for p in Field.get_syncpeaks(f)]


def _gpu_read(ctx, data, start, mtf=1.0):
    buf = np.frombuffer(data, np.uint8)
    ctx.set_capture(buf, buf.size, 0, 0)
    inf = ctx.decode_reads([start], [mtf])[0]
    ds = ctx.debug(0, 2, np.float64, int(inf.n_out))
    peaks = ctx.debug(0, 41, np.int32, 2048)[:max(int(inf.npeaks), 0)]
    return inf, ds, [int(p) for p in peaks]


def test_golden_read(gpu_ctx_ntsc):
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden
    from oracle.capture import FMT_U8, Capture
    from oracle.demod import RFDemod
    from oracle.field import FieldNTSC
    ctx, rf = gpu_ctx_ntsc
    data = make_golden.build_capture('ntsc_cav_u8_0p2s')
    start = 385743
    inf, ds, peaks = _gpu_read(ctx, data, start)
    orf = RFDemod(system='NTSC')
    raw = orf.demod(Capture(data, FMT_U8), start, 1000000, 1.0)
    f = FieldNTSC(orf, raw, 0, audio_offset=0)
    assert len(peaks) > 350                  # a sync pulse per line: 1,000,000 / 2,542 samples = 393 lines
    assert peaks == [int(p) for p in f.peaklist]
    assert peaks == _walk(ds, rf.linelen)
    assert inf.nvsync == len(f.vsyncs) > 0
    for q in range(inf.nvsync):
        assert list(inf.vsync[q]) == [int(x) for x in f.vsyncs[q]]
    assert inf.nextfieldoffset == f.nextfieldoffset
    ods = raw[0]['demod_sync']
    lv_err = np.abs(ds[peaks] - ods[peaks]).max() / max(np.abs(ods).max(), 1.0)
    med, tol = f.get_hsync_median()
    print('levels at the peaks: max rel diff %.3g; med_hsync %.17g (oracle %.17g)' % (lv_err, inf.med_hsync, med))
    assert lv_err < 1e-9
    assert abs(inf.med_hsync - med) <= 1e-9 * max(abs(med), 1.0)


def test_constant_samples(gpu_ctx_ntsc):
    ctx, rf = gpu_ctx_ntsc
    data = np.full(NSAMP, 128, np.uint8).tobytes()
    inf, ds, peaks = _gpu_read(ctx, data, 0)
    assert ds.size > 1000000
    assert np.all(ds == ds[0]), 'demod_sync of a constant capture is one value'
    assert not ds[0] > .2
    assert inf.npeaks == 0 and peaks == _walk(ds, rf.linelen) == []


def test_plateau_above_the_threshold(gpu_ctx_ntsc):
    ctx, rf = gpu_ctx_ntsc
    f_tip = rf.iretohz(-40)                       # mid-window of the sync detector (-55 .. -25 IRE)
    n = np.arange(NSAMP, dtype=np.float64)
    data = np.round(128 + 100 * np.sin(2 * np.pi * f_tip / 40e6 * n)).astype(np.uint8).tobytes()
    inf, ds, peaks = _gpu_read(ctx, data, 0)
    lo, hi = 200000, ds.size - 200000
    want = _walk(ds, rf.linelen)
    win = rf.linelen // 2
    ties = sum(1 for p in want if np.count_nonzero(ds[p:p + win] == ds[p]) > 1)
    print('demod_sync over [%d, %d): min %.17g max %.17g; %d peaks, %d of them with their level again later in the window'
          % (lo, hi, ds[lo:hi].min(), ds[lo:hi].max(), len(peaks), ties))
    assert ds[lo:hi].min() > .2, 'the detector is on throughout: every window has a peak'
    # a step of the walk is at most a window and a jump: 1271 + 1016 samples
    assert len(want) > (ds.size - 2 * rf.linelen) // (win + int(rf.linelen * .4))
    assert peaks == want
    # ties are decided here: windows whose maximum occurs again later in the window, the first one taken
    assert ties > 0
