"""The analog audio kernels stage by stage against the oracle, on the captures of
tests/audio_cases.py (runs through libldgpu.so on an MI355X): audio phase 1 (ldg_k_audio1: the
carrier slices, the 1024-point IFFT, fast_atan2, fold_tau, the block assembly and the zeroed
tail), phase 2 (ldg_k_audio2) and the 48 kHz downscale (ldg_k_audio_ds: the rounding and the clip).

Bars (DESIGN.md "Parity"): phase 1 and phase 2 within 1e-3 Hz on every sample, no exclusions
(test_audio_ref.py holds the reference's phase steps off the fold); counts and the next offset
exactly equal; the PCM equal except where the oracle's unrounded value lies within 2.5e-4 of a
half-integer, there within 1, on at most 4 samples of a field.
"""
import numpy as np
import pytest

import audio_cases as ac

pytestmark = pytest.mark.gpu

SLOT = 5          # below the fixtures' 8 read slots; nothing in this module keeps another read


def _ctx(request, system):
    return request.getfixturevalue('gpu_ctx_' + system.lower())[0]


def _decode(request, case, slot=SLOT):
    """The case's read decoded into `slot` of its system's session context."""
    from ldgpu import native
    r = ac.ref(case)
    ctx = _ctx(request, r.system)
    cap = ac.capture(case)
    ctx.set_capture(cap, cap.size, 0, 0)
    info = ctx.decode_reads([r.start], [1.0], slots=[slot])[0]
    assert info.status == native.FS_VALID and r.valid
    return ctx, r


def _check_phase1(ctx, slot, r):
    """-> the largest difference (Hz) of the two channels' phase-1 arrays, all samples."""
    worst = 0.0
    for ch in (0, 1):
        o = r.a1[ch]
        g = ctx.debug(slot, 12 + ch, np.float64, o.size)
        assert g.size == o.size
        assert np.all(g[r.nfill:] == 0.0) and r.nfill < o.size          # the tail past the last block
        d = float(np.abs(g - o).max())
        assert d < ac.HZ_TOL, (r.case, ch, d, int(np.abs(g - o).argmax()))
        worst = max(worst, d)
    return worst


def _check_phase2(ctx, slot, r):
    worst = 0.0
    for ch in (0, 1):
        o = r.a2[ch]
        g = ctx.debug(slot, 10 + ch, np.float64, o.size)
        assert g.size == o.size
        d = float(np.abs(g - o).max())
        assert d < ac.HZ_TOL, (r.case, ch, d, int(np.abs(g - o).argmax()))
        worst = max(worst, d)
    return worst


def _check_pcm(got, r, off):
    """One field's (pcm row, count, next offset) against downscale_audio at `off` -> the number
    of samples that differ (all of them near a rounding boundary, by 1)."""
    pcm, count, nxt = got
    o, onext, _ = r.ds[off]
    assert 2 * int(count) == o.size
    assert float(nxt) == float(onext)
    g = pcm[:o.size]
    near = r.near_half(off)
    assert int(near.sum()) <= ac.HALF_MAX
    diff = g.astype(np.int64) - o.astype(np.int64)
    assert np.all(diff[~near] == 0), (r.case, off, np.flatnonzero((diff != 0) & ~near)[:8])
    assert np.abs(diff).max() <= 1
    for level in (ac.CLIP, -ac.CLIP):                 # the clipped samples are the oracle's
        assert np.array_equal((g == level)[~near], (o == level)[~near])
    assert np.abs(g.astype(np.int64)).max() <= ac.CLIP
    assert not np.any(pcm[o.size:])                   # nothing written past the field's samples
    return int((diff != 0).sum())


@pytest.mark.parametrize('case', list(ac.CASES))
def test_phase1(case, request):
    """ldg_k_audio1's output (debug taps 12 / 13) against the oracle's assembled phase-1 array."""
    ctx, r = _decode(request, case)
    d = _check_phase1(ctx, SLOT, r)
    print('%s: audio phase 1 max |gpu - oracle| %.3e Hz over 2 x %d samples (fold margin %.2e rad)' % (
        case, d, r.a1[0].size, r.fold_margin()))


@pytest.mark.parametrize('case', list(ac.CASES))
def test_phase2(case, request):
    """ldg_k_audio2's output (debug taps 10 / 11) against the oracle's audio_phase2."""
    ctx, r = _decode(request, case)
    d = _check_phase2(ctx, SLOT, r)
    print('%s: audio phase 2 max |gpu - oracle| %.3e Hz over 2 x %d samples' % (case, d, r.a2[0].size))


@pytest.mark.parametrize('case', list(ac.CASES))
def test_downscale(case, request):
    """ldg_k_audio_ds against downscale_audio at three starting offsets: the sample count, the
    next offset, the rounding, the clip."""
    ctx, r = _decode(request, case)
    for off in ac.OFFSETS:
        pcm, counts, nxt = ctx.field_audio([SLOT], [off])
        k = _check_pcm((pcm[0], counts[0], nxt[0]), r, off)
        hi, lo = (int((pcm[0] == ac.CLIP).sum()), int((pcm[0] == -ac.CLIP).sum()))
        print('%s offset %g: %d of %d PCM samples differ (%d near a half-integer), %d at +%d, %d at -%d' % (
            case, off, k, 2 * counts[0], int(r.near_half(off).sum()), hi, ac.CLIP, lo, ac.CLIP))
    e = ac.CASES[case]['expect']['clip']
    pcm, counts, _ = ctx.field_audio([SLOT], [0.0])
    for ch, want in enumerate(e):
        x = pcm[0, ch:2 * counts[0]:2]
        if want == 'both':
            assert (x == ac.CLIP).any() and (x == -ac.CLIP).any()
        elif want == 'none':
            assert not (np.abs(x) == ac.CLIP).any()


def test_digital_silence_blocks(request):
    """Regression test for fold_tau at a phase step of exactly 0 (and fast_atan2 at (0, 0)): in the
    wholly blank demod blocks of the blank capture ldg_k_audio1 gives exactly audio_lowfreq, as the
    reference does -- `d <= 0` in fold_tau would give audio_lowfreq + freq_arf.  Only these
    samples are compared: the rest of this capture is ill-conditioned in the reference itself
    (audio_cases.BLANK)."""
    ctx, r = _decode(request, 'blank')
    low = r.rf.Filters['audio_lowfreq']
    for ch in (0, 1):
        z = r.a1[ch][:r.nfill] == low
        assert int(z.sum()) == 2 * 958
        g = ctx.debug(SLOT, 12 + ch, np.float64, r.a1[ch].size)[:r.nfill]
        assert np.all(g[z] == low), (ch, np.unique(g[z] - low)[:4])
        print('blank channel %d: %d samples of exactly audio_lowfreq, as the oracle' % (ch, int(z.sum())))


BATCH = ['loud', 'silent', 'drop']       # all NTSC
BATCH_SLOTS = [2, 6, 3]


def test_one_batch(request):
    """Three cases as the three reads of one decode_reads call, each in a slot of its own: every
    slot still matches its own oracle (the per-slot strides of aslice / audio1 / audio2 do not
    leak between reads), one field_audio call over the three gives each its PCM, and the field
    archive (archive_fields + archive_audio, strided and packed) returns field_audio's bytes.
    One decode_reads call reads one capture, so the capture here holds the three cases'
    captures one after another; read k starts at k * len + START and never leaves its own part
    (the demod's last block ends before START + 1,100,000)."""
    from ldgpu import native
    refs = [ac.ref(c) for c in BATCH]
    ctx = _ctx(request, 'NTSC')
    caps = [ac.capture(c) for c in BATCH]
    size = caps[0].size
    assert all(c.size == size for c in caps) and all(r.start == refs[0].start for r in refs)
    assert refs[0].start + ac.READLEN + 1 + refs[0].rf.blocklen <= size
    cap = np.concatenate(caps)
    ctx.set_capture(cap, cap.size, 0, 0)
    starts = [k * size + r.start for k, r in enumerate(refs)]
    infos = ctx.decode_reads(starts, [1.0] * 3, slots=BATCH_SLOTS)
    assert [i.status for i in infos] == [native.FS_VALID] * 3
    for case, slot, r in zip(BATCH, BATCH_SLOTS, refs):
        d1, d2 = _check_phase1(ctx, slot, r), _check_phase2(ctx, slot, r)
        print('%s in slot %d: phase 1 %.3e Hz, phase 2 %.3e Hz' % (case, slot, d1, d2))
    offs = ac.OFFSETS
    pcm, counts, nxt = ctx.field_audio(BATCH_SLOTS, offs)
    for k, r in enumerate(refs):
        n = _check_pcm((pcm[k], counts[k], nxt[k]), r, offs[k])
        print('%s in slot %d: %d PCM samples differ' % (BATCH[k], BATCH_SLOTS[k], n))
    # the archive: entries 3, 4, 5 (not the slots' numbers), read back in another order
    ctx.archive_fields(BATCH_SLOTS, 3)
    order = [2, 0, 1]
    ents, eoffs = [3 + k for k in order], [offs[k] for k in order]
    apcm, acounts, anxt = ctx.archive_audio(ents, eoffs)
    assert apcm.tobytes() == pcm[order].tobytes()
    assert np.array_equal(acounts, counts[order]) and np.array_equal(anxt, nxt[order])
    ppcm, pcounts, pnxt = ctx.archive_audio(ents, eoffs, packed=True)
    assert np.array_equal(pcounts, counts[order]) and np.array_equal(pnxt, nxt[order])
    assert ppcm.tobytes() == b''.join(pcm[k, :2 * counts[k]].tobytes() for k in order)

