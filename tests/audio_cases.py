"""Captures with hard analog audio carriers, and the oracle's reading of them (test infrastructure).

Every GPU test of the audio path elsewhere decodes ``SynthRF``'s fixed programme: 1 kHz (left) and
400 Hz (right) tones at +-50 kHz deviation.  The PCM then peaks at a third of full scale, the audio
filters see signal a few bins from DC only, and the phase steps of audio phase 1 stay 0.77 rad from
the fold at 0 and 2 pi.  The captures here take the synthesiser's video alone
(``SynthRF(system, first_frame=200, seed=31, audio=False)``, generated from sample 0 to
``START + 1,100,000`` in the parent's chunks of 2^22) and add the carriers themselves onto the float
RF, ``0.1 cos(2 pi frac(n fc / FS) + phase(n))`` with ``fc`` the system's ``audio_l`` / ``audio_r``;
then RF dropouts are overwritten with ``default_rng([31, 7, d0]).normal(0, 0.3, dn)`` (the
synthesiser's own draw), then ``SynthRF.quantise(rf, 'u8')``.  ldgpu/synth.py is not touched: the
golden captures pin its bytes.

A carrier is None (absent), ``('tone', fm, dev)``: phase = dev / fm sin(2 pi fm n / FS), or
``('programme', k, dev)``: white noise ``default_rng([5, k])`` at FS / 256, low-passed to 20 kHz by
``firwin(129)``, normalised to peak 1, interpolated linearly to FS, times ``dev``; the phase is
2 pi cumsum(deviation) / FS.

``CASES`` is the table; each case is one read, ``RFDemod.demod(cap, START, 1000000, 1.0)`` followed by
``FieldNTSC`` / ``FieldPAL``.  ``expect`` holds what the case exists for, asserted on the oracle by
test_audio_ref.py; test_audio_gpu.py holds the HIP kernels to the oracle stage by stage (audio
phase 1, phase 2, the 48 kHz downscale) on every case.

  clip      'both': PCM samples at +32766 and at -32766 on that channel; 'none': no sample at
            either; 'any': not claimed (noise, which may or may not reach the clip)
  span      channels whose phase-1 output spans more than half of freq_arf (no carrier: the
            demodulated phase steps of noise cover the whole circle)
"""
import contextlib
import io
import os
import sys

import numpy as np
import scipy.signal as sps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, 'ld-decode_amd'), os.path.join(HERE, 'golden')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ldgpu.synth import FS, NTSC, PAL, SynthRF  # noqa: E402

from damage import BASE, READLEN, START, TAIL  # noqa: E402

TAU = 2 * np.pi
CHANNELS = ('audio_left', 'audio_right')
OFFSETS = [0.0, 1.0e-5, 2.05e-5]       # downscale_audio's starting time offsets (s) tested per case
CLIP = 32766

# ---- the bars (DESIGN.md "Parity") -----------------------------------------------------------
HZ_TOL = 1e-3                          # audio phase 1 and phase 2 against the oracle, Hz, every sample
# Phase 1 near the fold: a phase step within round-off of 0 or 2 pi may fold to either end of
# [0, 2 pi] and the two differ by freq_arf.  The reference's steps keep at least FOLD_MARGIN rad
# away (above 3e-4 rad measured on every case, the GPU's round-off there is of order 1e-12 rad),
# so the comparison needs no exclusions.
FOLD_MARGIN = 1e-6
# The PCM is equal wherever the oracle's unrounded value is further than HALF_MARGIN from a half-
# integer: HZ_TOL * 32767 / 150000 = 2.18e-4, times a wow factor of at most 1.15.  Within it the
# rounding may go either way (a difference of 1), on at most HALF_MAX samples of a field.
HALF_MARGIN = 2.5e-4
HALF_MAX = 4


def _wow():
    import make_golden
    return make_golden.wow('NTSC', 0.0015, 0.002)      # the components of ntsc_cav_u8_wow_0p2s


def _case(system, left, right, dropouts=(), blank=(), wow=False, **expect):
    return dict(system=system, carriers=(left, right), dropouts=tuple(dropouts), blank=tuple(blank), wow=wow,
                expect=expect)


N, P = 'NTSC', 'PAL'
LOUD = (('tone', 1000.0, 170000.0), ('tone', 400.0, 160000.0))
CASES = {
    # both clip signs on both channels, and the rounding right at the clip
    'loud': _case(N, *LOUD, clip=('both', 'both'), span=()),
    # no carrier at all: fast_atan2 at small magnitudes, fold_tau over the whole circle
    'silent': _case(N, None, None, clip=('any', 'any'), span=(0, 1)),
    # one carrier: the channels are independent (the halves of the ldg_k_audio1 workgroup, ch in ldg_k_audio2)
    'one_side': _case(P, ('tone', 1000.0, 165000.0), None, clip=('both', 'any'), span=(1,)),
    # modulation at the top of the audio band: audio_lpf2's roll-off, the carrier filters' skirts
    'high': _case(P, ('tone', 15000.0, 100000.0), ('tone', 19000.0, 60000.0), clip=('none', 'none'), span=()),
    # every audio bin carries signal at once
    'programme_ntsc': _case(N, ('programme', 0, 140000.0), ('programme', 1, 140000.0), clip=('none', 'none'), span=()),
    'programme_pal': _case(P, ('programme', 0, 140000.0), ('programme', 1, 140000.0), clip=('none', 'none'), span=()),
    # the standard tones with noise bursts inside a live carrier, block boundaries inside a dropout
    'drop': _case(N, ('tone', 1000.0, 50000.0), ('tone', 400.0, 50000.0), dropouts=((600000, 3000), (900000, 40000)),
                  clip=('none', 'none'), span=(0, 1)),
    # the loud carriers on a capture with time-base error: swow != 1 multiplied in before the clip
    'wow_loud': _case(N, *LOUD, wow=True, clip=('both', 'both'), span=(), wow_min=1e-3),
}


# Not in the table: the standard tones with a span of digital silence (the RF exactly 0, u8 128) that
# holds two whole demod blocks.  Their carrier slices are exactly 0, atan2(0, 0) = 0 and every phase
# step is exactly 0, which the reference leaves at 0: the one place where fold_tau's `d < 0` differs
# from `d <= 0` (by freq_arf).  Nothing rounds there, so those samples are compared exactly.  The rest
# of this capture is ill-conditioned in the reference itself and is held to nothing: in the blocks that
# are blank in part the filtered signal decays to round-off level, where the phase is noise.  Measured
# on the oracle with 1e-12 of noise added to the samples: the line locations 192..206 move by up to 4.5
# samples (`drop`, noise in the same span: 2e-11), so a GPU decode differs there as well (phase 1 by up
# to 5e-3 Hz on 126 samples, three line locations by up to 7.5 samples, one PCM sample).
BLANK = {'blank': _case(N, ('tone', 1000.0, 50000.0), ('tone', 400.0, 50000.0), blank=((900000, 40000),),
                        zero_steps=2 * 2 * 958)}


def _phase(spec, k_n):
    """The modulating phase of a carrier at samples 0 .. k_n - 1."""
    kind, a, dev = spec
    if kind == 'tone':
        return (dev / a) * np.sin(TAU * a * (np.arange(k_n) / FS))
    # programme
    m = k_n // 256 + 2
    taps = sps.firwin(129, 20000.0 / (FS / 256 / 2))
    x = np.convolve(np.random.default_rng([5, int(a)]).normal(0.0, 1.0, m + 128), taps, mode='valid')
    x /= np.abs(x).max()
    sig = np.interp(np.arange(k_n) / 256.0, np.arange(m), x)
    return TAU * np.cumsum(dev * sig) / FS


def build(case):
    """The capture of a case: u8 samples 0 .. START + TAIL as a numpy array."""
    c = (CASES.get(case) or BLANK[case]) if isinstance(case, str) else case
    p = NTSC if c['system'] == 'NTSC' else PAL
    g = SynthRF(system=c['system'], audio=False, wow=_wow() if c['wow'] else (), **BASE)
    total, parts = START[c['system']] + TAIL, []
    while g.pos < total:
        parts.append(g.generate(min(1 << 22, total - g.pos)))
    rf = np.concatenate(parts)
    n = np.arange(total, dtype=np.int64)
    for fc, spec in zip((p['audio_l'], p['audio_r']), c['carriers']):
        if spec is not None:
            rf += 0.1 * np.cos(TAU * np.mod(n * (fc / FS), 1.0) + _phase(spec, total))
    for d0, dn in c['dropouts']:
        rf[d0:d0 + dn] = np.random.default_rng([BASE['seed'], 7, d0]).normal(0.0, 0.3, dn)
    for d0, dn in c['blank']:
        rf[d0:d0 + dn] = 0.0
    return SynthRF.quantise(rf, 'u8')


class Ref:
    """The oracle's decode of a case, without the video: ``a1`` / ``a2`` the phase-1 (2.5 MHz,
    as assembled from the blocks) and phase-2 (625 kHz) audio per channel, ``nfill`` the phase-1
    samples the blocks wrote (zeros follow), the field's validity, final line locations and line
    count, and per offset of OFFSETS downscale_audio's (pcm, next offset, unrounded values)."""

    def __init__(self, case):
        from oracle.capture import FMT_U8, Capture
        from oracle.field import FieldNTSC, FieldPAL, downscale_audio
        from damage import _rf
        c = CASES.get(case) or BLANK[case]
        self.case, self.system, self.start = case, c['system'], START[c['system']]
        rf = self.rf = _rf(self.system)
        video, a1, a2 = rf.demod_stages(Capture(capture(case), FMT_U8), self.start, READLEN, 1.0)
        raw = (video, a2)
        with contextlib.redirect_stdout(io.StringIO()):
            f = (FieldNTSC if self.system == 'NTSC' else FieldPAL)(rf, raw, 0, audio_offset=0)
        self.a1 = [a1[ch] for ch in CHANNELS]
        self.a2 = [a2[ch] for ch in CHANNELS]
        self.valid = bool(f.valid)
        self.skip_reason = f.skip_reason
        self.nfill = int(max(np.flatnonzero(a).max() for a in self.a1)) + 1
        self.ds = {}
        if self.valid:
            self.linecount = f.linecount
            self.linelocs = np.asarray(f.linelocs, dtype=np.float64)
            self.dsaudio, self.audio_next_offset = f.dsaudio, f.audio_next_offset
            for off in OFFSETS:
                self.ds[off] = downscale_audio(raw[1], f.linelocs, rf, f.linecount, off, unrounded=True)

    # ---- what the read exercised --------------------------------------------------------
    def fold_margin(self):
        """The smallest distance (rad) of a kept phase-1 phase step from 0 and from 2 pi, over
        the steps that are not exactly 0 (zero_steps counts those: blocks of digital silence)."""
        F = self.rf.Filters
        m = np.inf
        for a in self.a1:
            u = a[:self.nfill] - F['audio_lowfreq']
            u = u[u != 0.0] * (TAU / F['freq_arf'])
            m = min(m, float(u.min()), float((TAU - u).min()))
        return m

    def zero_steps(self):
        """The kept phase-1 samples, both channels, whose phase step is exactly 0."""
        return sum(int((a[:self.nfill] == self.rf.Filters['audio_lowfreq']).sum()) for a in self.a1)

    def span(self, ch):
        a = self.a1[ch][:self.nfill]
        return float(a.max() - a.min()) / self.rf.Filters['freq_arf']

    def clipped(self, ch, off=0.0):
        """(samples at +CLIP, samples at -CLIP) of a channel."""
        x = self.ds[off][0][ch::2]
        return int((x == CLIP).sum()), int((x == -CLIP).sum())

    def near_half(self, off):
        """Mask over the interleaved PCM: the unrounded value lies within HALF_MARGIN of a half-integer."""
        r = self.ds[off][2]
        return np.abs(r - np.floor(r) - 0.5) <= HALF_MARGIN

    def wow_range(self):
        """The largest |swow - 1| over the field's lines."""
        return float(np.abs(np.diff(self.linelocs[:self.linecount + 2]) / self.rf.linelen - 1).max())


_CAP, _REF = {}, {}


def capture(case):
    """build(case), once per process (1.5 MB a case)."""
    if case not in _CAP:
        _CAP[case] = build(case)
    return _CAP[case]


def ref(case):
    """Ref(case), once per process (a Ref holds no video: about 1.3 MB)."""
    if case not in _REF:
        _REF[case] = Ref(case)
    return _REF[case]
