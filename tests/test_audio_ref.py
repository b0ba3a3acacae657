"""The captures of tests/audio_cases.py do in the oracle what they exist for (CPU only): the
field is valid, the clip is reached (or not), an absent carrier demodulates to the whole circle,
and the two conditions hold that let test_audio_gpu.py compare without exclusions -- no phase-1
phase step near the fold, almost no PCM value near a rounding boundary."""
import numpy as np
import pytest

import audio_cases as ac


@pytest.mark.parametrize('case', list(ac.CASES))
def test_case_does_its_job(case):
    r = ac.ref(case)
    e = ac.CASES[case]['expect']
    assert r.valid, r.skip_reason
    n1 = r.a1[0].size
    assert r.a1[1].size == n1 and r.nfill < n1                   # a zeroed tail exists
    assert all(np.all(a[r.nfill:] == 0.0) for a in r.a1)
    assert r.a2[0].size == r.a2[1].size == n1 // 4
    for off in ac.OFFSETS:
        for ch, want in enumerate(e['clip']):
            hi, lo = r.clipped(ch, off)
            if want == 'both':
                assert hi >= 10 and lo >= 10, (off, ch, hi, lo)
            elif want == 'none':
                assert hi == 0 and lo == 0, (off, ch, hi, lo)
    for ch in (0, 1):
        if ch in e['span']:
            assert r.span(ch) > 0.5, (ch, r.span(ch))
        else:
            assert r.span(ch) < 0.25, (ch, r.span(ch))
    if 'wow_min' in e:
        assert r.wow_range() >= e['wow_min']                      # swow is not 1
    print('%s: clipped L %r R %r, span %.3f %.3f, |swow - 1| <= %.2e' % (
        case, r.clipped(0), r.clipped(1), r.span(0), r.span(1), r.wow_range()))


@pytest.mark.parametrize('case', list(ac.CASES))
def test_phase_steps_keep_off_the_fold(case):
    """Every kept phase-1 phase step lies at least FOLD_MARGIN from 0 and 2 pi, so the kernel's
    elementwise fold and the reference's unwrap + fold loops agree up to round-off."""
    r = ac.ref(case)
    m, z = r.fold_margin(), r.zero_steps()
    print('%s: smallest fold margin %.3g rad, %d steps exactly 0' % (case, m, z))
    assert m >= ac.FOLD_MARGIN and z == 0


@pytest.mark.parametrize('case', list(ac.CASES))
def test_few_values_at_a_rounding_boundary(case):
    """At most HALF_MAX unrounded values of a field within HALF_MARGIN of a half-integer; the
    unrounded values are the PCM's (rounded half to even, clipped on int32)."""
    r = ac.ref(case)
    for off in ac.OFFSETS:
        pcm, nxt, raw = r.ds[off]
        assert raw.size == pcm.size and pcm.dtype == np.int16
        assert np.array_equal(np.clip(np.round(raw).astype(np.int32), -ac.CLIP, ac.CLIP), pcm)
        k = int(r.near_half(off).sum())
        print('%s offset %g: %d of %d values near a half-integer' % (case, off, k, pcm.size))
        assert k <= ac.HALF_MAX
    assert np.array_equal(r.ds[0.0][0], r.dsaudio) and r.ds[0.0][1] == r.audio_next_offset


def test_digital_silence_gives_steps_of_exactly_zero():
    """The blank capture (audio_cases.BLANK): its two wholly blank demod blocks give 958 kept
    phase-1 samples each, per channel, of exactly audio_lowfreq -- a phase step of exactly 0,
    left at 0 by the reference's fold loops -- in one run, and nowhere else."""
    r = ac.ref('blank')
    assert r.valid and r.zero_steps() == ac.BLANK['blank']['expect']['zero_steps']
    for a in r.a1:
        z = np.flatnonzero(a[:r.nfill] == r.rf.Filters['audio_lowfreq'])
        assert z.size == 2 * 958 and z[-1] - z[0] == z.size - 1


def test_stages_are_the_demod():
    """demod_stages() hands out what demod() computes: the same video and phase-2 audio, and
    the phase-1 array that audio_phase2 turns into it."""
    from oracle.capture import FMT_U8, Capture
    r = ac.ref('high')
    cap = Capture(ac.capture('high'), FMT_U8)
    video, a2 = r.rf.demod(cap, r.start, ac.READLEN, 1.0)
    for ch, k in enumerate(ac.CHANNELS):
        assert np.array_equal(a2[k], r.a2[ch])
    again = r.rf.audio_phase2(dict(zip(ac.CHANNELS, r.a1)))
    for ch, k in enumerate(ac.CHANNELS):
        assert np.array_equal(again[k], r.a2[ch])
