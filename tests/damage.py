"""Captures with damaged sync pulses, and the oracle's reading of them (test infrastructure).

The damage model works on the baseband: ``DamagedRF`` overwrites the synthesiser's composite
IRE over given spans before the FM modulation, so that sync pulses can be erased (0 IRE),
moved, added (sync-tip level), made too shallow or too deep, or widened into broad pulses.
An edit is ``(absolute line, duration in lines, IRE)`` and covers the samples
``a <= n < a + dur * spl`` with ``a = (line - start_line) * spl``; edits apply in order, so a
pulse written after an erasure of the same span survives.  RF ``dropouts`` (the carrier
replaced by noise) are still the parent's.  Every capture is ``SynthRF(system, first_frame=200,
seed=31)`` otherwise at its defaults, u8, generated in the parent's chunks of 2^22 samples
from sample 0 to the last read start + 1,100,000, so its bytes are deterministic.

``CASES`` is the table: per case the system, the edits and / or dropouts, the read starts
(each read is one ``RFDemod.demod(cap, start, 1000000, 1.0)`` + ``FieldNTSC`` / ``FieldPAL``), what
the oracle makes of each read (``expect``, asserted on the CPU by test_damage_ref.py) and, in the
comment above it, the branch of ``Field.__init__`` and of csrc/field.hip it exists for.
test_damage_gpu.py holds the HIP kernels to the oracle's Field on every read of the table.

``skip_reason == 'linelocs'`` (LDG_FS_LINELOCS) is reached, by ``linelocs_ntsc`` / ``linelocs_pal``,
through the KeyError of the tail extrapolation (field.hip: "linelocs2[prev_valid - 1] KeyError").  Its
other exits are reached by nothing tried in the oracle and stay untested: a line number outside
-1024..1023, a fill with no valid neighbour on either side, and an exception of the hsync refinement
(candidates: a second interval a few lines after the first, ``vs_near``; hsyncs only in the second
half of the field, ``first_half``; both decode as valid fields).  See DESIGN.md "Parity".
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, 'ld-decode_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from ldgpu.synth import NTSC, PAL, SynthRF  # noqa: E402

READLEN = 1000000
TAIL = 1100000                       # capture samples kept past the last read start
BASE = dict(first_frame=200, seed=31)
START = {'NTSC': 385743, 'PAL': 508767}


class DamagedRF(SynthRF):
    """SynthRF whose composite IRE is overwritten over ``edits`` (see the module docstring)."""

    def __init__(self, edits=(), **kw):
        super().__init__(**kw)
        self.edits = tuple((float(line), float(dur), float(ire)) for line, dur, ire in edits)

    def _ire(self, n):
        return self._apply_edits(n, super()._ire(n))

    def _apply_edits(self, n, ire):
        for line, dur, level in self.edits:
            a = (line - self.t0_lines) * self.spl
            b = a + dur * self.spl
            # n ascends (sample indices, or the disc time of a capture with time-base error)
            i0, i1 = np.searchsorted(n, a, 'left'), np.searchsorted(n, b, 'left')
            if i0 < i1:
                ire[i0:i1] = level
        return ire


def _units(system):
    H = (NTSC if system == 'NTSC' else PAL)['line_us']
    return 4.7 / H, 2.35 / H, 0.5 - 4.7 / H          # HS, EQ, BR in lines


def erase_hsync(system, lines):
    HS, _, _ = _units(system)
    return [(l, 1.3 * HS, 0.0) for l in lines]


def erase_eq(system, halflines):
    _, EQ, _ = _units(system)
    return [(l, 1.3 * EQ, 0.0) for l in halflines]


def pulses(system, lines, width='hs', ire=None):
    HS, EQ, BR = _units(system)
    w = {'hs': HS, 'eq': EQ, 'br': BR}.get(width, width)
    tip = -40.0 if system == 'NTSC' else -43.0
    return [(l, w, tip if ire is None else ire) for l in lines]


def fake_interval(system, line):
    """A whole vertical interval written from ``line`` on: the hsyncs under it erased, then
    pre-equalizing, broad and post-equalizing pulses on the half-line grid (6 + 6 + 6 half-lines
    NTSC, 5 + 5 + 5 PAL)."""
    n = 6 if system == 'NTSC' else 5
    half = [line + k / 2 for k in range(3 * n)]
    return (erase_hsync(system, [line + k for k in range((3 * n + 1) // 2 + 1)]) +
            pulses(system, half[:n], 'eq') + pulses(system, half[n:2 * n], 'br') + pulses(system, half[2 * n:], 'eq'))


def _r(n):
    return list(range(n))


def _case(system, edits=(), dropouts=(), reads=None, expect=None, **kw):
    reads = [START[system]] if reads is None else list(reads)
    expect = expect if isinstance(expect, list) else [expect] * len(reads)
    assert len(expect) == len(reads)
    return dict(system=system, edits=list(edits), dropouts=tuple(dropouts), reads=reads, expect=expect, **kw)


def X(outcome='valid', **kw):
    """What the oracle makes of one read.  outcome: valid / no_vsync / short / tbc / linelocs /
    crash.  Optional claims: nvsync, log (the printed lines that matter, exactly), bad_min (a
    lower bound on the bad lines outside the clean read's), framenr_none, nfo_moved (True:
    nextfieldoffset differs from the clean read's), peaks ('more' / 'fewer' than the clean
    read's, or an exact count), fills (the gap-fill paths of compute_linelocs that run:
    'head', 'interior', 'tail'), votes (the vote repairs made: 'next', 'prev'), vsync0 (the first vsync row)."""
    return dict(outcome=outcome, **kw)


N, P = 'NTSC', 'PAL'
VOTE = 'vsync vote needed %d'
NOVS = 'no/corrupt VSYNC found, jumping forward'
DROPOUTS = ((1741434, 15000), (4420767, 15000))     # tests/test_cli.py DROPOUT_CAPTURE

CASES = {}


def build(case):
    """The capture of a case: u8 samples 0 .. last read start + TAIL as a numpy array."""
    c = CASES[case] if isinstance(case, str) else case
    g = DamagedRF(system=c['system'], edits=c['edits'], dropouts=c['dropouts'], **BASE)
    left, parts = max(c['reads']) + TAIL, []
    while left > 0:
        n = min(1 << 22, left)
        parts.append(SynthRF.quantise(g.generate(n), 'u8'))
        left -= n
    return np.concatenate(parts)


class Read:
    """The oracle's decode of one read: ``field`` (None after a ReferenceCrash), ``outcome``,
    the lines it printed, and the demod it worked on."""

    def __init__(self, system, data, start, mtf=1.0):
        from oracle.capture import FMT_U8, Capture
        from oracle.demod import ReferenceCrash
        from oracle.field import FieldNTSC, FieldPAL
        self.system, self.start = system, start
        self.rf = _rf(system)
        self.raw = self.rf.demod(Capture(data, FMT_U8), start, READLEN, mtf)
        buf = io.StringIO()
        self.field, self.crash = None, None
        with contextlib.redirect_stdout(buf):
            try:
                self.field = (FieldNTSC if system == 'NTSC' else FieldPAL)(self.rf, self.raw, 0, audio_offset=0)
            except ReferenceCrash as e:
                self.crash = str(e)
        if self.field is None:
            # the peak list the constructor had found before it raised
            from oracle.field import Field
            g = Field.__new__(Field)
            g.data, g.rf, g.start, g.inlinelen = self.raw, self.rf, 0, self.rf.linelen
            self.crash_peaks = g.get_syncpeaks()
        self.log = buf.getvalue().splitlines()
        f = self.field
        self.outcome = 'crash' if f is None else ('valid' if f.valid else f.skip_reason)

    # -- what the read exercised (for the coverage assertions) ---------------------------
    def raw_votes(self):
        """determine_field's votes of the vsyncs found, before the repair."""
        f = self.field
        return [f.determine_field(int(v[0]))[1] for v in f.vsyncs]

    def vote_repairs(self):
        """'next' / 'prev' per zero vote that the repair took from the next / previous vsync."""
        v = self.raw_votes()
        out = set()
        if len(v) < 2:
            return out
        for i, x in enumerate(v):
            if x == 0:
                if i < len(v) - 1 and v[i + 1] != 0:
                    out.add('next')
                elif i >= 1 and v[i - 1] != 0:
                    out.add('prev')
        return out

    def line_numbers(self):
        """The line numbers compute_linelocs gives the regular peaks (the keys of its dict)."""
        f = self.field
        pl, locs, lens = f.peaklist, set(), [f.inlinelen]
        prev_i = prev_n = None
        for i in range(0, int(f.vsyncs[1][1])):
            med = np.median(lens[-25:])
            if not f.is_regular_hsync(i):
                continue
            if prev_i is None:
                num = int(np.round((pl[i] - pl[int(f.vsyncs[0][1])]) / med))
            elif 0.98 <= (pl[i] - pl[prev_i]) / f.inlinelen <= 1.02:
                lens.append(pl[i] - pl[prev_i])
                num = prev_n + 1
            else:
                num = prev_n + int(np.round((pl[i] - pl[prev_i]) / med))
            locs.add(num)
            prev_i, prev_n = i, num
        return locs

    def fills(self):
        """The gap-fill paths of compute_linelocs this field runs: 'head' (no valid line
        before), 'interior' (between two), 'tail' (none after)."""
        f, locs, out = self.field, self.line_numbers(), set()
        for l in range(1, f.linecount + 5):
            if l in locs:
                continue
            pv = any(i in locs for i in range(l, -10, -1))
            nv = any(i in locs for i in range(l, f.linecount + 1))
            out.add('head' if not pv else ('interior' if nv else 'tail'))
        return out

    def bad_lines(self):
        return set(np.nonzero(np.asarray(self.field.linebad, dtype=bool))[0].tolist())


    def facts(self):
        """The read in small: what test_damage_ref.py asserts on (no sample arrays)."""
        f = self.field
        d = dict(outcome=self.outcome, log=[l for l in self.log if l.startswith('vsync vote needed') or l == NOVS])
        if f is None:
            d['npeaks'] = len(self.crash_peaks)
            return d
        d.update(npeaks=len(f.peaklist), nvsync=len(f.vsyncs), vsyncs=[[int(x) for x in v] for v in f.vsyncs],
                 nfo=int(f.nextfieldoffset), votes=self.vote_repairs() if len(f.vsyncs) else set())
        if self.outcome in ('valid', 'tbc'):
            d.update(fills=self.fills(), bad=self.bad_lines())
        if self.outcome == 'valid':
            d['framenr'] = f.vbi['framenr']
        return d


_RF, _CAP, _FACTS = {}, {}, {}


def _rf(system):
    from oracle.demod import RFDemod
    if system not in _RF:
        _RF[system] = RFDemod(system=system)
    return _RF[system]


def capture(case):
    """build(case), once per process (only the latest is kept: a capture is 1.5 to 5.5 MB)."""
    if case not in _CAP:
        _CAP.clear()
        _CAP[case] = build(case)
    return _CAP[case]


def oracle_read(case, k):
    """Read k of a case through the oracle (not kept: a Read holds the whole demod)."""
    c = CASES[case]
    r = Read(c['system'], capture(case), c['reads'][k])
    _FACTS.setdefault((case, k), r.facts())
    return r


def facts(case, k):
    """Read.facts() of read k of a case, computed once per process."""
    if (case, k) not in _FACTS:
        oracle_read(case, k)
    return _FACTS[(case, k)]


def clean_facts(system, start):
    """The facts of the undamaged capture's read at the same start (None: the clean case has no such read)."""
    name = 'clean_' + system.lower()
    return facts(name, CASES[name]['reads'].index(start)) if start in CASES[name]['reads'] else None


def _table():
    T = {}
    two = {'interior', 'tail'}
    # ---- NTSC.  The read at 385743 starts at line 251.7; its vertical interval runs from line
    # 262.5 (6 + 6 + 6 half-lines), the next from line 525; hsyncs stand on the whole lines from 272 on.
    # The read at 1052829 is the next of the oracle's chain: it starts on a sync peak (peak 0 at sample 0).
    # the undamaged capture: what the other cases are compared with (the last five lines are a tail fill)
    T['clean_ntsc'] = _case(N, reads=[385743, 1052829], expect=X(nvsync=2, log=[], fills=two, votes=set()))
    # three hsyncs missing: an interior gap fill, linebad from compute_linelocs
    T['erase3'] = _case(N, erase_hsync(N, [300 + k for k in _r(3)]), expect=X(peaks='fewer', bad_min=3, fills=two))
    # a sync-level pulse mid-line: a regular peak whose gap is not accepted and rounds to no new line
    T['fake_mid'] = _case(N, pulses(N, [350.5]), expect=X(peaks='more', bad_new=0))
    # a pulse 0.12 lines after an hsync: two peaks get one line number, the last write wins
    T['fake_close'] = _case(N, pulses(N, [350.12]), expect=X(peaks='same', bad_min=1))
    # 30 hsyncs 0.06 lines late: gaps outside .98..1.02, numbered by the running median of the last 25 lengths
    T['shift_run'] = _case(N, erase_hsync(N, [400 + k for k in _r(30)]) + pulses(N, [400.06 + k for k in _r(30)]),
                           expect=X(peaks='same', bad_min=30))
    # 60 hsyncs 0.3 lines late: the same path with the hsync refinement rejecting every one of them
    T['shift_big'] = _case(N, erase_hsync(N, [400 + k for k in _r(60)]) + pulses(N, [400.3 + k for k in _r(60)]),
                           expect=X(peaks='same', bad_min=60))
    # syncs too shallow (-20 IRE) and too deep (-70 IRE) for the sync slicer: no peaks there
    T['shallow_deep'] = _case(N, pulses(N, [420 + k for k in _r(4)], ire=-20) + pulses(N, [430 + k for k in _r(4)], ire=-70),
                              expect=X(peaks='fewer', bad_min=8))
    # six broad pulses mid-field with no equalizing pulses before them: > .9 peaks that are no vsync candidates
    T['fake_vsync'] = _case(N, pulses(N, [380 + k / 2 for k in _r(6)], 'br'), expect=X(nvsync=2, peaks='more', bad_min=4))
    # a whole vertical interval mid-field: three vsyncs, a zero vote repaired from the next one, vsyncs[1] mid-field
    T['three_vs'] = _case(N, fake_interval(N, 380),
                          expect=X(nvsync=3, log=[VOTE % 1], votes={'next'}, nfo_moved=True, bad_min=140))
    # ten hsyncs three times as wide: five vsyncs, zero votes repaired from the next and from the previous one
    T['wide_sync'] = _case(N, pulses(N, [300 + k for k in _r(10)], 3 * _units(N)[0]),
                           expect=X(nvsync=5, log=[VOTE % 1, VOTE % 2, VOTE % 3], votes={'next', 'prev'}, nfo_moved=True))
    # every other equalizing pulse of the read's interval missing: vote 0 on vsync 0, line0 = vsync - 7, no VBI
    T['eq_alt'] = _case(N, erase_eq(N, [262.5 + k for k in _r(3)] + [268.5 + k for k in _r(3)]),
                        expect=X(nvsync=2, log=[VOTE % 0], votes={'next'}, framenr_none=True, peaks='fewer'))
    # the same in both intervals: two zero votes with nothing to repair them from
    T['eq_alt_both'] = _case(N, erase_eq(N, [b + k for b in (262.5, 268.5, 525.5, 531.5) for k in _r(3)]),
                             expect=X(nvsync=2, log=[VOTE % 0, VOTE % 1], votes=set(), framenr_none=True, nfo_moved=True))
    # no pre-equalizing pulses before the first interval: one vsync, `short`, jumpto a real peak
    T['no_eq_pre'] = _case(N, erase_eq(N, [262.5 + k / 2 for k in _r(6)]), expect=X('short', nvsync=1, log=[]))
    # the second interval blanked: `short` with peaklist[vsyncs[0][1] - 10] = peaklist[0]
    T['kill_vs2'] = _case(N, [(525 + k / 2, 0.5, 0.0) for k in _r(18)], expect=X('short', nvsync=1, log=[], nfo=1024))
    # all four equalizing groups missing: `no_vsync` with >= 200 peaks (no candidate survives)
    T['no_eq_both2'] = _case(N, erase_eq(N, [b + k / 2 for b in (262.5, 268.5, 525, 531) for k in _r(6)]),
                             expect=X('no_vsync', nvsync=0))
    # every hsync of the field missing: `no_vsync` through the < 200 peaks exit
    T['hs_all'] = _case(N, erase_hsync(N, [272 + k for k in _r(245)]), expect=X('no_vsync', nvsync=0))
    # the first 12 hsyncs after the interval missing: the fill reaches into lines 0..9 (never bad), no VBI
    T['erase_head'] = _case(N, erase_hsync(N, [272 + k for k in _r(12)]), expect=X(bad_min=11, framenr_none=True))
    # the last 20 hsyncs missing: the sequential tail extrapolation over 25 lines, an earlier nextfieldoffset
    T['erase_tail'] = _case(N, erase_hsync(N, [505 + k for k in _r(20)]), expect=X(bad_min=20, nfo_moved=True, fills=two))
    # half a field of hsyncs missing, at its start and at its end.  first_half's bad lines are extrapolated with a
    # short gap, so one line of linelocs2 is 24,448 samples long: the burst pass has to resample a line of any length
    T['first_half'] = _case(N, erase_hsync(N, [272 + k for k in _r(118)]), expect=X(bad_min=118, framenr_none=True))
    T['last_half'] = _case(N, erase_hsync(N, [403 + k for k in _r(122)]), expect=X(bad_min=122, nfo_moved=True))
    # a sync-level pulse in the middle of 100 lines: 100 more peaks, none of them a new line
    T['double'] = _case(N, pulses(N, [300.5 + k for k in _r(100)]), expect=X(peaks='more', bad_new=0))
    # four hsyncs of five missing: the burst refinement raises, `tbc`
    T['erase_most'] = _case(N, erase_hsync(N, [275 + k for k in _r(245) if k % 5]), expect=X('tbc', nvsync=2, nfo_moved=True))
    # reads that start inside the interval's reach: the vsync lies within the first 11 peaks, the reference raises
    T['crash_ntsc'] = _case(N, reads=[403800, 410000], expect=X('crash'))
    # the boundary of that test: the latest start with the vsync at peak 11 (403800 has it at peak 10)
    T['k11_ntsc'] = _case(N, reads=[401300], expect=X(nvsync=2, vsync0=[11, 4, 0]))
    # the 10 hsyncs before the interval narrowed to equalizing width, the last two post-equalizing pulses
    # missing: vote 0, vsyncs[0][1] = vsync - 7 is an irregular peak with no regular one in the nine lines
    # before it, so lines 1..9 are filled backwards from the first hsync after the interval (head fill)
    T['head_ntsc'] = _case(N, erase_hsync(N, [253 + k for k in _r(10)]) + pulses(N, [253 + k for k in _r(10)], 'eq') +
                           erase_eq(N, [271, 271.5]), expect=X(log=[VOTE % 0], votes={'next'}, fills={'head', 'tail'}))
    # the chain's second read with its second interval blanked: `short` with peaklist[0] == 0, the jump of 240 lines
    T['novs_ntsc'] = _case(N, [(787.5 + k / 2, 0.5, 0.0) for k in _r(18)], reads=[1052829], expect=X('short', nvsync=1, log=[NOVS]))
    # a second vertical interval three lines after the first: three vsyncs, vsyncs[1] a few lines into the read
    T['vs_near'] = _case(N, fake_interval(N, 275), expect=X(nvsync=3, log=[VOTE % 1], votes={'next'}, nfo_moved=True,
                                                            framenr_none=True))
    # LDG_FS_LINELOCS (the tail extrapolation's KeyError): the first interval without post-equalizing pulses
    # and a second one right after it, so both vsyncs share line0 and no regular peak lies between them; the
    # hsync two lines before line0 missing, so the only valid neighbour (line -1) has no line before it
    T['linelocs_ntsc'] = _case(N, erase_hsync(N, [260]) + erase_eq(N, [268.5 + k / 2 for k in _r(6)]) + fake_interval(N, 272),
                               expect=X('linelocs', nvsync=3, log=[VOTE % 0]))
    # the RF dropouts of tests/test_cli.py's capture, at the reads of the oracle's chain that print
    T['rf_dropouts'] = _case(N, dropouts=DROPOUTS, reads=[1701096, 3722163, 4332243],
                             expect=[X(log=[VOTE % 0], votes={'next'}, framenr_none=True), X('short', nvsync=1, log=[NOVS]),
                                     X('short', nvsync=1, log=[])])
    # ---- PAL.  The read at 508767 starts at line 298.7; its vertical interval runs from line 310 (5 + 5 + 5
    # half-lines), the next from line 622.5 (5 + 5 + 10); hsyncs stand on the whole lines from 318 on, sync tip
    # -43 IRE.  The undamaged read already needs a vote (repaired from the previous vsync); the next read of
    # the chain, at 1311072, needs one repaired from the next.
    T['clean_pal'] = _case(P, reads=[508767, 1311072], expect=[X(nvsync=2, log=[VOTE % 1], votes={'prev'}, fills=two),
                                                                X(nvsync=2, log=[VOTE % 0], votes={'next'}, fills=two)])
    T['p_erase3'] = _case(P, erase_hsync(P, [400 + k for k in _r(3)]), expect=X(peaks='fewer', bad_min=3))
    T['p_fake_close'] = _case(P, pulses(P, [400.12]), expect=X(peaks='same', bad_min=1))
    T['p_shift_run'] = _case(P, erase_hsync(P, [400 + k for k in _r(30)]) + pulses(P, [400.06 + k for k in _r(30)]),
                             expect=X(peaks='same', bad_min=30))
    T['p_shallow_deep'] = _case(P, pulses(P, [420 + k for k in _r(4)], ire=-20) + pulses(P, [430 + k for k in _r(4)], ire=-75),
                                expect=X(peaks='fewer', bad_min=8))
    T['p_double'] = _case(P, pulses(P, [350.5 + k for k in _r(100)]), expect=X(peaks='more'))
    # three vsyncs, the fake one with a non-zero vote: the last one's zero vote is repaired from it
    T['p_three_vs'] = _case(P, fake_interval(P, 450), expect=X(nvsync=3, log=[VOTE % 2], votes={'prev'}, nfo_moved=True, bad_min=170))
    T['p_vs_near'] = _case(P, fake_interval(P, 321), expect=X(nvsync=3, log=[VOTE % 2], nfo_moved=True, framenr_none=True))
    # five vsyncs, three of them with the same line0
    T['p_wide_sync'] = _case(P, pulses(P, [350 + k for k in _r(10)], 3 * _units(P)[0]),
                             expect=X(nvsync=5, log=[VOTE % 4], votes={'prev'}, nfo_moved=True))
    T['p_eq_alt'] = _case(P, erase_eq(P, [310 + k for k in _r(3)] + [315 + k for k in _r(3)]), expect=X(nvsync=2, peaks='fewer', bad_min=5))
    T['p_eq_alt2'] = _case(P, erase_eq(P, [622.5 + k for k in _r(3)] + [627.5 + k for k in _r(3)]), expect=X(nvsync=2, log=[], votes=set()))
    T['p_no_eq_pre'] = _case(P, erase_eq(P, [310 + k / 2 for k in _r(5)]), expect=X('short', nvsync=1, log=[]))
    T['p_kill_vs2'] = _case(P, [(622.5 + k / 2, 0.5, 0.0) for k in _r(15)], expect=X('short', nvsync=1, log=[], nfo=1024))
    T['p_no_eq_both'] = _case(P, erase_eq(P, [b + k / 2 for b in (310, 315, 622.5, 627.5) for k in _r(5)]),
                              expect=X('no_vsync', nvsync=0))
    # four hsyncs of five missing: `no_vsync` with < 200 peaks; two of three: the pilot refinement or the
    # resampling raises, `tbc`; one of two: still valid, 150 lines filled
    T['p_erase_most'] = _case(P, erase_hsync(P, [320 + k for k in _r(290) if k % 5]), expect=X('no_vsync', nvsync=0))
    T['p_erase_most3'] = _case(P, erase_hsync(P, [320 + k for k in _r(290) if k % 3]), expect=X('tbc', nvsync=2))
    T['p_erase_most2'] = _case(P, erase_hsync(P, [320 + k for k in _r(290) if k % 2]), expect=X(bad_min=140, framenr_none=True))
    T['p_erase_head'] = _case(P, erase_hsync(P, [318 + k for k in _r(12)]), expect=X(bad_min=11))
    T['p_erase_tail'] = _case(P, erase_hsync(P, [600 + k for k in _r(22)]), expect=X(bad_min=22, nfo_moved=True, fills=two))
    T['p_first_half'] = _case(P, erase_hsync(P, [318 + k for k in _r(140)]), expect=X(bad_min=139, framenr_none=True))
    T['p_last_half'] = _case(P, erase_hsync(P, [480 + k for k in _r(142)]), expect=X(bad_min=142, nfo_moved=True))
    T['crash_pal'] = _case(P, reads=[524427, 536000], expect=X('crash'))
    T['k11_pal'] = _case(P, reads=[521867], expect=X(nvsync=2, vsync0=[11, 5, 1]))
    # as head_ntsc; an equalizing pulse added at line 317.5 makes the vote 0 (PAL: exactly one long gap)
    T['head_pal'] = _case(P, erase_hsync(P, [300 + k for k in _r(10)]) + pulses(P, [300 + k for k in _r(10)], 'eq') +
                          pulses(P, [317.5], 'eq'), expect=X(log=[VOTE % 0, VOTE % 1], votes=set(), fills={'head', 'tail'}))
    T['novs_pal'] = _case(P, [(935 + k / 2, 0.5, 0.0) for k in _r(15)], reads=[1311072], expect=X('short', nvsync=1, log=[NOVS]))
    T['linelocs_pal'] = _case(P, erase_hsync(P, [307]) + erase_eq(P, [315 + k / 2 for k in _r(5)]) + fake_interval(P, 318),
                              expect=X('linelocs', nvsync=3, log=[VOTE % 2]))
    return T


CASES.update(_table())


def check_claims(case, k):
    """Assert what the table claims of read k of a case on the oracle's decode of it."""
    c = CASES[case]
    e, got = c['expect'][k], facts(case, k)
    assert got['outcome'] == e['outcome'], (case, k, got['outcome'])
    clean = clean_facts(c['system'], c['reads'][k])
    for key, want in e.items():
        if key == 'outcome':
            continue
        if key in ('nvsync', 'log', 'votes', 'nfo'):
            assert got[key] == want, (case, k, key, got[key])
        elif key == 'vsync0':
            assert got['vsyncs'][0] == want, (case, k, got['vsyncs'])
        elif key == 'fills':
            assert want <= got['fills'], (case, k, got['fills'])
        elif key == 'framenr_none':
            assert got['framenr'] is None, (case, k, got['framenr'])
        elif key == 'peaks':
            d = got['npeaks'] - clean['npeaks']
            assert (d > 0) if want == 'more' else (d < 0) if want == 'fewer' else d == 0, (case, k, got['npeaks'])
        elif key == 'nfo_moved':
            assert got['nfo'] != clean['nfo'], (case, k, got['nfo'])
        elif key == 'bad_min':
            assert len(got['bad'] - clean['bad']) >= want, (case, k, sorted(got['bad'] - clean['bad']))
        elif key == 'bad_new':
            assert len(got['bad'] - clean['bad']) == want, (case, k, sorted(got['bad'] - clean['bad']))
        else:
            raise KeyError(key)


# ---- whole captures for the decode loop (test_damage_gpu.py) ----------------------------------
# Several damages in different fields of one capture, so that the planner's predictions fail at
# them.  NTSC: frames start at line 525 k, vertical intervals at 525 k and 525 k + 262.5; PAL: frames
# at 625 k, intervals at 625 k + 310 and 625 k + 622.5.  Every capture's first read (sample 0, mid-field)
# is `short`.  A `no_vsync` field moves the reference one second on, past the end of a capture of
# this length, where its demod raises: it stands in `ntsc_crash` only.
def _ntsc_whole():
    return (erase_eq(N, [1050 + k / 2 for k in _r(6)]) +                  # two `short` reads, one jumping 240 lines
            fake_interval(N, 1695) +                                        # three vsyncs, nextfieldoffset mid-field
            erase_hsync(N, [2113 + k for k in _r(245) if k % 5]))           # `tbc`


def _pal_whole():
    return (fake_interval(P, 2025) +                                        # three vsyncs
            erase_hsync(P, [2510 + k for k in _r(290) if k % 3]))           # `tbc`


CRASH_AT = 5000847 + 40000000        # where the reference reads on after the `no_vsync` field of ntsc_crash
WHOLE = {
    'ntsc_cav': dict(system=N, clv=False, seconds=0.25, edits=_ntsc_whole(), want={'short', 'tbc', 'three_vs'}),
    'ntsc_clv': dict(system=N, clv=True, seconds=0.25, edits=_ntsc_whole(), want={'short', 'tbc', 'three_vs'}),
    'pal_cav': dict(system=P, clv=False, seconds=0.25, edits=_pal_whole(), want={'tbc', 'three_vs'}),
    # the intervals at lines 2100 and 2362.5 without equalizing pulses: the read at 4390767 is `short` and jumps
    # 240 lines, the read at 5000847 is `no_vsync` and the reference reads on one second later, at line
    # 17801.4; a vertical interval written at line 17804 puts a vsync within
    # that read's first 11 peaks, where the reference raises.  Only the samples up to 0.2 s and around
    # the second read are synthesised; between them the capture repeats its first 4,000,000 samples.
    'ntsc_crash': dict(system=N, clv=False, seconds=0.2, tail=(CRASH_AT - 150000, 1300000),
                       edits=erase_eq(N, [b + k / 2 for b in (2100, 2106, 2362.5, 2368.5) for k in _r(6)]) +
                       fake_interval(N, 17804), want=set()),
}


def build_whole(name):
    """The u8 bytes of a whole capture of WHOLE."""
    w = WHOLE[name]
    kw = dict(system=w['system'], edits=w['edits'], clv=w['clv'], **BASE)
    g = DamagedRF(**kw)
    left, parts = int(40e6 * w['seconds']), []
    while left > 0:
        n = min(1 << 22, left)
        parts.append(SynthRF.quantise(g.generate(n), 'u8'))
        left -= n
    head = np.concatenate(parts)
    if 'tail' not in w:
        return head.tobytes()
    t0, tn = w['tail']
    g = DamagedRF(**kw)
    g.pos = t0                               # (the filters start afresh there: a transient of a few samples)
    tail = SynthRF.quantise(g.generate(tn), 'u8')
    gap = np.resize(head[:4000000], t0 - head.size)
    return np.concatenate([head, gap, tail]).tobytes()


_WHOLE = {}


def oracle_whole(name):
    """oracle.framer.decode_capture of a whole capture, once per process: dict(data, frames, pcm,
    meta, fields = a dict per Field of the completed frames in read order, crashed = False or the
    ReferenceCrash's message).  Where the oracle
    raises ReferenceCrash, what it had produced before (its decode loop run again over that many frames)."""
    if name not in _WHOLE:
        from oracle.capture import FMT_U8
        from oracle.demod import ReferenceCrash
        from oracle.framer import decode_capture
        w = WHOLE[name]
        data = build_whole(name)
        fields, done = [], []
        crashed = False

        def note(f):         # (not the Field: it holds the read's whole demod)
            fields.append(dict(readsample=int(f.readsample), outcome='valid' if f.valid else f.skip_reason,
                               nvsync=len(f.vsyncs), nextfieldoffset=int(f.nextfieldoffset)))

        with contextlib.redirect_stdout(io.StringIO()):
            try:
                frames, pcm, meta = decode_capture(data, FMT_U8, system=w['system'], on_field=note,
                                                   log=lambda *a: done.append(a) if a and a[0] == 'frame ' else None)
            except ReferenceCrash as e:
                crashed = str(e)
                del fields[:]
                frames, pcm, meta = decode_capture(data, FMT_U8, system=w['system'], length=len(done), on_field=note)
        _WHOLE[name] = dict(data=data, frames=frames, pcm=pcm, meta=meta, fields=fields, crashed=crashed)
    return _WHOLE[name]
