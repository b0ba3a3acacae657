"""Captures with damaged and unusual Philips code lines, and the oracle's reading of them (test
infrastructure, modelled on tests/damage.py whose START, BASE, READLEN, TAIL and Read it reuses).

``VbiRF`` is a ``DamagedRF`` whose code words come from a table (three arbitrary 24-bit words per
frame, or one word for one line of one field) and which rewrites single code lines of the baseband:
a cell held flat, a 25th cell, the whole train moved, cells >= k delayed, the swing reduced, the
line left flat; ``edits`` and RF ``dropouts`` are the parents'.  Every capture is otherwise
``SynthRF(system, first_frame=200, seed=31)``, u8, in chunks of 2^22 samples from sample 0 to the
read start + 1,100,000.

``CASES`` is the table: per case the system, the words, the damage, the read start (one read each,
at damage.START: field 1 of capture frame 0), what the oracle makes of it (``expect``: the three
lines' codes, their crossing counts, the vbi members; asserted on the CPU by test_vbi_ref.py
together with the robustness condition, ``robust``) and, above it, the branch of
decodephillipscode / processphilipscode and of ldg_k_philips (csrc/field.hip) it exists for.
``WHOLE`` holds the captures for the decode loop.  test_vbi_gpu.py holds the kernel and
GPUDecoder to the oracle on both.

Exits reached by nothing tried in the oracle, which stay untested (DESIGN.md "Parity"):
  * the gap rejection at 24 crossings (`np.min(gaps) > 1.85 and np.max(gaps) < 2.15`): each search
    window is 1.9..2.1 us after the last crossing, plus one sample of interpolation; every gap of
    every line of the table lies in 1.97..2.08 us (delays of 0.0 to 0.3 us were bisected, see `delay`;
    test_vbi_ref.py asserts it of every line that has 24 crossings);
  * the kernel's `n + 1 > 100000` guard: a line has room for fewer than 30 cells;
  * `py_index` failing (LDG_FS_CRASH): the code lines lie 16..21 lines after the first vsync, which a
    field that gets this far has at peak 11 or later and at least 240 lines before the end of the read.
    Tried: the latest starts that still decode (damage.py's k11_ntsc / k11_pal, 401300 and 521867), where
    the first code line begins at sample 54,095 / 64,725; a negative index needs a crossing within 20
    samples of the read's start, and Python's negative index would wrap, not raise.
"""
import contextlib
import copy
import io

import numpy as np

import damage as D
from damage import BASE, READLEN, START, TAIL, DamagedRF, Read  # noqa: F401
from ldgpu.synth import NTSC, PAL, SynthRF

N, P = 'NTSC', 'PAL'
# the frame lines (0-based, per field) that carry the words: the three lines the decoder reads
CODE_LINES = {N: NTSC['code_lines'], P: ((17, 18, 19), (329, 330, 331))}
KINDS = ('word', 'flat', 'flat_cell', 'extra', 'shift', 'delay', 'swing')


class TableCodes:
    """A FrameCodes whose words come from a table {frame k: (w0, w1, w2)}, any 24-bit values;
    frames not in the table keep the base's."""

    def __init__(self, base, table):
        self.base, self.table = base, {int(k): tuple(int(w) for w in v) for k, v in table.items()}
        assert all(len(v) == 3 and all(0 <= w < 1 << 24 for w in v) for v in self.table.values())

    def __getattr__(self, name):
        return getattr(self.base, name)

    def codes(self, k):
        return self.table.get(k, None) or self.base.codes(k)


class VbiRF(DamagedRF):
    """DamagedRF with table-driven code words and per-line damage of the code waveform.

    words: {frame k: (w0, w1, w2)} for both fields of frame k.  lines: {(k, field, j): spec} for
    code line j (0..2) of field 0 / 1 of frame k; spec is a dict of
      word=w            this line's word (a per-field difference),
      flat=ire          no train: the line's picture span held at that level,
      flat_cell=(c, ire) cell c held at that level,
      extra=bit         a 25th cell with that bit after cell 23,
      shift=d           the whole train d us late (negative: early),
      delay=(c, d)      cells >= c start d us late (the level before them held meanwhile),
      swing=a           the train between 0 and a IRE.
    The train is written wherever its cells fall inside the line, over sync and burst too.
    The parent's `edits` apply after it, its RF `dropouts` to the modulated carrier."""

    def __init__(self, words=None, lines=None, **kw):
        super().__init__(**kw)
        self.codes = TableCodes(self.codes, words or {})
        self.p = dict(self.p, code_lines=CODE_LINES[self.p['system']])
        self.lines = {}
        for (k, fld, j), spec in (lines or {}).items():
            assert set(spec) <= set(KINDS), spec
            self.lines[(int(k), int(fld), int(j))] = dict(spec)

    def _ire(self, n):
        ire = SynthRF._ire(self, n)
        if self.lines:
            self._code_lines(n, ire)
        return self._apply_edits(n, ire)

    def _code_lines(self, n, ire):
        p = self.p
        H, L = p['line_us'], p['lines']
        la = n / self.spl + self.t0_lines
        fl = np.floor(la).astype(np.int64)              # absolute line, ascending
        for (k, fld, j), spec in self.lines.items():
            line = k * L + p['code_lines'][fld][j]
            i0, i1 = np.searchsorted(fl, line, 'left'), np.searchsorted(fl, line, 'right')
            if i0 == i1:
                continue
            tau = (la[i0:i1] - fl[i0:i1]) * H
            seg = ire[i0:i1]
            if fld in self.code_fields:
                seg[(tau >= 10.0) & (tau < 58.0)] = 0.0          # the parent's train
            if 'flat' in spec:
                seg[(tau >= 5.0) & (tau < H - 1.5)] = spec['flat']          # (over the burst too)
                continue
            word = spec.get('word', self.codes.codes(k)[j])
            ncell = 25 if 'extra' in spec else 24
            bits = np.array([(word >> (23 - i)) & 1 for i in range(24)] + [int(spec.get('extra', 0))])
            t = tau - 10.0 - spec.get('shift', 0.0)
            if 'delay' in spec:
                c, d = spec['delay']
                t = np.where(t >= 2.0 * c + d, t - d, np.where(t >= 2.0 * c, np.nextafter(2.0 * c, 0.0), t))
            cell = np.floor(t / 2.0).astype(np.int64)
            inside = (cell >= 0) & (cell < ncell)
            cc = cell[inside]
            second = (t[inside] - 2.0 * cc) >= 1.0
            out = np.where(np.where(bits[cc] == 1, second, ~second), float(spec.get('swing', 100.0)), 0.0)
            if 'flat_cell' in spec:
                c, level = spec['flat_cell']
                out[cc == c] = level
            seg[inside] = out


def scan(field, l, demod=None):
    """decodephillipscode's crossing search on code line l, on the field's demod or another:
    (the number of crossings found, the method's own return value, the smallest and largest gap in us)."""
    from oracle.field import calczc
    g = copy.copy(field)
    if demod is not None:
        g.data = ({'demod': demod},)
    data = g.data[0]['demod']
    thr = g.rf.iretohz(50)
    cur = calczc(data, int(g.linelocs[l] + g.usectoinpx(2)), thr, count=int(g.usectoinpx(12)))
    zc = []
    while cur is not None:
        zc.append(cur)
        cur = calczc(data, cur + g.usectoinpx(1.9), thr, count=int(g.usectoinpx(0.2)))
    gaps = g.inpxtousec(np.diff(zc))
    return len(zc), g.decodephillipscode(l), ((float(gaps.min()), float(gaps.max())) if len(zc) > 1 else None)


def _hex(code):
    return None if code is None else ''.join('%X' % x for x in code)


class VRead(Read):
    """damage.Read with what the oracle's VBI decode made of the three code lines."""

    def facts(self):
        f = self.field
        d = dict(outcome=self.outcome)
        if self.outcome != 'valid':
            return d
        lines = self.rf.SysParams['philips_codelines']
        sc = [scan(f, l) for l in lines]
        assert [c for _, c, _ in sc] == [f.linecode[l] for l in lines]
        d.update(codes=[_hex(c) for _, c, _ in sc], n=[n for n, _, _ in sc], gaps=[g for _, _, g in sc],
                 vbi={k: v for k, v in f.vbi.items() if v is not None and v is not False},
                 linelocs=[float(f.linelocs[l]) for l in lines], robust=robust(f))
        return d


def robust(f):
    """The robustness condition: the three lines decode to the same codes with the same crossing
    counts on the demod plus 1e-6 max|demod|, minus it, and plus seeded uniform noise of that
    amplitude (the GPU demod is held to 1e-9 of full scale)."""
    lines = f.rf.SysParams['philips_codelines']
    demod = np.asarray(f.data[0]['demod'], dtype=np.float64)
    a = 1e-6 * np.abs(demod).max()
    base = [scan(f, l)[:2] for l in lines]
    noise = np.random.default_rng(20240607).uniform(-a, a, demod.size)
    return all([scan(f, l, demod + p)[:2] for l in lines] == base for p in (a, -a, noise))


CASES = {}
_CAP, _FACTS = {}, {}


def generator(c, lines=True):
    return VbiRF(system=c['system'], words=c['words'], lines=c['lines'] if lines else None,
                 edits=c['edits'] if lines else (), dropouts=c['dropouts'] if lines else (), **BASE)


def build(case, lines=True):
    """The capture of a case: u8 samples 0 .. last read start + TAIL (lines=False: the same
    words without the per-line damage, the edits and the dropouts)."""
    c = CASES[case] if isinstance(case, str) else case
    g = generator(c, lines)
    left, parts = max(c['reads']) + TAIL, []
    while left > 0:
        n = min(1 << 22, left)
        parts.append(SynthRF.quantise(g.generate(n), 'u8'))
        left -= n
    return np.concatenate(parts)


def capture(case):
    if case not in _CAP:
        _CAP.clear()
        _CAP[case] = build(case)
    return _CAP[case]


def oracle_read(case, k=0):
    c = CASES[case]
    r = VRead(c['system'], capture(case), c['reads'][k])
    _FACTS.setdefault((case, k), r.facts())
    return r


def facts(case, k=0):
    if (case, k) not in _FACTS:
        oracle_read(case, k)
    return _FACTS[(case, k)]


def E(codes, n, **vbi):
    """What the oracle makes of the read: the three lines' codes ('-': None) and crossing counts,
    and the members of Field.vbi that are neither None nor False."""
    return dict(outcome='valid', codes=[None if c == '-' else c for c in codes.split()], n=list(n), vbi=vbi)


def _lines(fld=1, k=0, **kw):
    return {(k, fld, int(name[1])): spec for name, spec in kw.items()}


def _c(system, words, expect, lines=None, **kw):
    return D._case(system, expect=expect, words={0: tuple(words)}, lines=lines or {}, **kw)


F = 0xF80345                         # picture number 345: cells 0..4 are ones, cell 23 is a one
US = {N: NTSC['line_us'], P: PAL['line_us']}


def _table():
    T = {}
    # ---- NTSC, the read at 385743: field 1 of frame 0, code lines 279..281 (linelocs 16..18) ----
    # Crossing count.  decodephillipscode `len(zc) == 24` false / ldg_k_philips `n == 24` false.
    # A flat cell 0 (at 0 IRE) and a flat cell 23 leave 23 crossings; a flat cell 12 (at 100 IRE) ends the
    # chain of 0.2 us windows after 12
    T['flat_cells'] = _c(N, (F, F, F), E('- - -', (23, 12, 23)),
                         _lines(j0=dict(flat_cell=(0, 0.0)), j1=dict(flat_cell=(12, 100.0)), j2=dict(flat_cell=(23, 0.0))))
    # a 25th cell, a one and a zero: 25 crossings (the loop runs past bit 23: `n < 24` guards the shift)
    T['extra_cell'] = _c(N, (F, F, F), E('- - F80345', (25, 25, 24), framenr=345), _lines(j0=dict(extra=1), j1=dict(extra=0)))
    # no crossing at all: the first search returns None (kernel: rc != 0 at once, n = 0).  A white line
    # from before the search start, a train that stays under the 50 IRE threshold, a train 8 us late
    # (its first crossing past the 12 us window)
    T['no_crossings'] = _c(N, (F, F, F), E('- - -', (0, 0, 0)),
                           _lines(j0=dict(flat=100.0), j1=dict(swing=35.0), j2=dict(shift=8.0)))
    # a train 8.7 us early, over sync and burst: the search starts inside it and finds its last 22 crossings
    T['early'] = _c(N, (F, F, F), E('F80345 - F80345', (24, 22, 24), framenr=345), _lines(j1=dict(shift=-8.7)))
    # one line valid between two malformed ones: the interpretation skips `lc is None` / `!s_ok[q]`
    T['one_valid'] = _c(N, (F, F, F), E('- F80345 -', (5, 24, 25), framenr=345),
                        _lines(j0=dict(flat_cell=(5, 100.0)), j2=dict(extra=1)))
    # part of a line overwritten with 0 IRE (a DamagedRF edit over cells 5..8), and an RF dropout of 15 us
    # across the next line
    T['edit_part'] = _c(N, (F, F, F), E('- - F80345', (5, 7, 24), framenr=345),
                        edits=[(279 + 20 / US[N], 8 / US[N], 0.0)], dropouts=((458600, 600),))
    # Timing.  The 0.2 us window after 1.9 us (calczc count = int(0.2 us) / `1.9 * fr`, `py_int(0.2 * fr)`):
    # cells 12.. delayed.  Bisected in the oracle: line 0 flips between 0.0797 and 0.0820 us, line 1 between
    # 0.0727 and 0.0750 (the flip depends on the crossing's sample phase).  Inside on line 0, outside on line 1
    T['delay'] = _c(N, (F, F, F), E('F80345 - F80345', (24, 12, 24), framenr=345),
                    _lines(j0=dict(delay=(12, 0.058)), j1=dict(delay=(12, 0.097))))
    # the whole train late.  Bisected: line 0 flips between 6.479 and 6.482 us, line 1 between 6.4995 and
    # 6.503: what is lost first is the 24th crossing, which runs into the next line's sync (23 crossings);
    # the first crossing leaves the 12 us window only further on (`no_crossings`)
    T['late'] = _c(N, (F, F, F), E('F80345 - F80345', (24, 23, 24), framenr=345),
                   _lines(j0=dict(shift=6.45), j1=dict(shift=6.53)))
    # Bit patterns.  All zeros: the line rises at each cell start, the search locks onto the cell boundaries and
    # reads 24 ones; all ones; alternating (every nibble A / 5)
    T['patterns_a'] = _c(N, (0x000000, 0xFFFFFF, 0xAAAAAA), E('FFFFFF FFFFFF AAAAAA', (24, 24, 24), framenr=86665))
    # 0x555555 and a first cell 0 followed by a one: the boundary lock-in ends after one crossing
    T['patterns_b'] = _c(N, (0x555555, 0x7F8123, 0xF8ABCD), E('- - F8ABCD', (1, 1, 24), framenr=11233))
    # Interpretation (processphilipscode / thread 0 of ldg_k_philips).
    # `lc[0] == 15 and lc[2] == 13`: hours 0, 1, 9; `lc[2] == 0xE`: second nibble >= 10 and < 10 (negative
    # seconds, which the record must keep apart from VBI_NONE); `h == 0x87ffff`
    T['clv_h0'] = _c(N, (0xF0DD07, 0x8AE345, 0x87FFFF), E('F0DD07 8AE345 87FFFF', (24, 24, 24), minutes=7, seconds=3, clvframe=45, isclv=True))
    T['clv_h1'] = _c(N, (0xF1DD07, 0x82E345, 0x87FFFF), E('F1DD07 82E345 87FFFF', (24, 24, 24), minutes=67, seconds=-77, clvframe=45, isclv=True))
    T['clv_h9'] = _c(N, (0xF9DD59, 0x8FE959, 0x8DC123), E('F9DD59 8FE959 8DC123', (24, 24, 24), minutes=599, seconds=59, clvframe=59,
                                                          status=0x8DC123, isclv=True))
    # 0x87FFFF alone makes the field CLV; lead-in 0x88FFFF falls through every branch
    T['clv_only'] = _c(N, (0x8DC123, 0x87FFFF, 0x88FFFF), E('8DC123 87FFFF 88FFFF', (24, 24, 24), status=0x8DC123, isclv=True))
    # `lc[0] == 15`: the `& 7` mask on 0xFF (79999), 0xF0 with non-BCD digits, 0xF8; status 0x8BAxxx; the stop
    # code 0x82CFFF and a chapter code 0x8nnDDD fall through
    T['pic_ff'] = _c(N, (0x88FFFF, 0x8BA777, 0xFF9999), E('88FFFF 8BA777 FF9999', (24, 24, 24), framenr=79999, status=0x8BA777))
    T['pic_f0'] = _c(N, (0x812DDD, 0x82CFFF, 0xF0ABCD), E('812DDD 82CFFF F0ABCD', (24, 24, 24), framenr=11233))
    # lead-out 0x80EEEE is read as seconds / picture (-86, 154) and makes the field CLV next to a picture number
    T['leadout'] = _c(N, (0x80EEEE, F, 0x8BA777), E('80EEEE F80345 8BA777', (24, 24, 24), seconds=-86, clvframe=154, framenr=345,
                                                   status=0x8BA777, isclv=True))
    # the same kind of code on several lines: the later line wins
    T['later_pic'] = _c(N, (F, 0xF80346, 0xF80347), E('F80345 F80346 F80347', (24, 24, 24), framenr=347))
    T['later_status'] = _c(N, (0x8BA111, 0x8DC222, 0x8BA333), E('8BA111 8DC222 8BA333', (24, 24, 24), status=0x8BA333))
    T['later_clv'] = _c(N, (0xF1DD07, 0xF2DD15, 0x8AE345), E('F1DD07 F2DD15 8AE345', (24, 24, 24), minutes=135, seconds=3, clvframe=45, isclv=True))
    # ---- PAL, the read at 508767: field 1 of frame 0, whose linelocs 19..21 are the frame lines 329..331
    # (0-based).  synth.py's PAL `code_lines` are (18, 19, 20) and (331, 332, 333): one and two lines later
    # than the lines the decoder reads (17..19 and 329..331), so of a default capture this read sees only word
    # 0, on its third line, and the other field's reads see words 0 and 1 on their second and third.  It is the
    # numbering, not the read's field parity; the golden captures keep it, VbiRF writes the lines that are read.
    T['p_counts'] = _c(P, (F, F, F), E('- - -', (23, 25, 0)),
                       _lines(j0=dict(flat_cell=(23, 0.0)), j1=dict(extra=1), j2=dict(swing=35.0)))
    # bisected: the delay flips between 0.0750 and 0.0773 us on line 0, 0.0492 and 0.0516 on line 1; the late
    # shift between 6.923 and 6.927 on line 0, 6.899 and 6.903 on line 1
    T['p_delay'] = _c(P, (F, F, F), E('F80345 - F80345', (24, 12, 24), framenr=345),
                      _lines(j0=dict(delay=(12, 0.052)), j1=dict(delay=(12, 0.075))))
    T['p_late'] = _c(P, (F, F, F), E('F80345 - -', (24, 23, 2), framenr=345),
                     _lines(j0=dict(shift=6.895), j1=dict(shift=6.93), j2=dict(shift=-8.7)))
    T['p_patterns'] = _c(P, (0x000000, 0x555555, 0x7F8123), E('FFFFFF - -', (24, 1, 1), framenr=86665))
    T['p_clv'] = _c(P, (0xF1DD07, 0x82E345, 0x87FFFF), E('F1DD07 82E345 87FFFF', (24, 24, 24), minutes=67, seconds=-77, clvframe=45, isclv=True))
    T['p_leadout'] = _c(P, (0x80EEEE, F, 0x8BA777), E('80EEEE F80345 8BA777', (24, 24, 24), seconds=-86, clvframe=154, framenr=345,
                                                     status=0x8BA777, isclv=True))
    T['p_other'] = _c(P, (0x88FFFF, 0x8DC123, 0xFF9999), E('88FFFF 8DC123 FF9999', (24, 24, 24), framenr=79999, status=0x8DC123))
    return T


CASES.update(_table())


def branches(fa):
    """The interpretation branches the read's codes take, and its crossing-count classes."""
    out = set()
    for c, n in zip(fa['codes'], fa['n']):
        out.add('n0' if n == 0 else 'n<24' if n < 24 else 'n24' if n == 24 else 'n>24')
        if c is None:
            out.add('none')
            continue
        h = int(c, 16)
        if c[0] == 'F' and c[2] == 'D':
            out.add('minutes')
        elif c[0] == 'F':
            out.add('framenr')
        else:
            hit = False
            if c[2] == 'E':
                out.add('seconds>=10' if int(c[1], 16) >= 10 else 'seconds<10')
                hit = True
            if h >> 12 in (0x8dc, 0x8ba):
                out.add('status_%x' % (h >> 12))
                hit = True
            if h == 0x87ffff:
                out.add('87ffff')
                hit = True
            if not hit:
                out.add('other')
    return out


# ---- whole captures for the decode loop (test_vbi_gpu.py) --------------------------------------
# NTSC, capture frame k starts at line 525 k; a capture starts at line 100 of frame 0, so the decode's
# frame i is made of the two fields of capture frame i + 1 (top field: code lines 16..18, field 0).
def _blank(k, fld, js=(0, 1, 2)):
    return {(k, fld, j): dict(flat=0.0) for j in js}


def _whole():
    from ldgpu.synth import STATUS_CODE, cav_code, clv_minutes_code
    W = {}
    # no codes in either field of frame 3, codes only in the second field of frame 4
    W['cav_gaps'] = dict(clv=False, seconds=0.3, words={}, lines={**_blank(3, 0), **_blank(3, 1), **_blank(4, 0)})
    # 201, 202, 9000, 204, ...: the MTF level goes 0.98 -> 0.1 -> 0.98
    W['cav_jump'] = dict(clv=False, seconds=0.3, words={3: (cav_code(9000), cav_code(9000), STATUS_CODE)}, lines={})
    # frame 3: seconds nibble 2 (< 10) next to minutes 0: seconds -74; frame 4: minutes 0 in the first field, 5 in
    # the second
    W['clv_odd'] = dict(clv=True, seconds=0.3, words={3: (0xF0DD00, 0x82E615, 0x87FFFF)},
                        lines={(4, 1, 0): dict(word=clv_minutes_code(5))})
    # both minutes lines of frame 3 flat: seconds without minutes
    W['clv_no_minutes'] = dict(clv=True, seconds=0.25, words={}, lines={**_blank(3, 0, (0,)), **_blank(3, 1, (0,))})
    # lead-out on the second code line of frame 3: seconds -86 without minutes
    W['cav_leadout'] = dict(clv=False, seconds=0.25, words={3: (cav_code(203), 0x80EEEE, STATUS_CODE)}, lines={})
    return W


WHOLE = _whole()
CRASHES = ('clv_no_minutes', 'cav_leadout')


def build_whole(name):
    w = WHOLE[name]
    g = VbiRF(system=N, clv=w['clv'], words=w['words'], lines=w['lines'], **BASE)
    left, parts = int(40e6 * w['seconds']), []
    while left > 0:
        n = min(1 << 22, left)
        parts.append(SynthRF.quantise(g.generate(n), 'u8'))
        left -= n
    return np.concatenate(parts).tobytes()


_WHOLE = {}


def oracle_whole(name):
    """oracle.framer.decode_capture of a whole capture, once per process, as damage.oracle_whole:
    dict(data, frames, pcm, meta, fields, crashed).  `fields` has, per Field of the completed frames in
    read order, its read start, MTF level, parity and vbi dict.  Where the oracle's loop raises
    TypeError (mergevbi: `None * 60 * fps`), `crashed` is its message and the rest is what the loop had
    produced before (run again over that many frames)."""
    if name not in _WHOLE:
        from oracle.capture import FMT_U8
        from oracle.framer import decode_capture
        data = build_whole(name)
        fields, done = [], []
        crashed = False

        def note(f):
            fields.append(dict(readsample=int(f.readsample), valid=bool(f.valid), mtf=float(f.mtf_level),
                               istop=bool(f.istop) if f.valid else None, vbi=dict(f.vbi) if f.valid else None))

        with contextlib.redirect_stdout(io.StringIO()):
            try:
                frames, pcm, meta = decode_capture(data, FMT_U8, system=N, on_field=note,
                                                   log=lambda *a: done.append(a) if a and a[0] == 'frame ' else None)
            except TypeError as e:
                crashed = str(e)
                del fields[:]
                frames, pcm, meta = decode_capture(data, FMT_U8, system=N, length=len(done), on_field=note)
        _WHOLE[name] = dict(data=data, frames=frames, pcm=pcm, meta=meta, fields=fields, crashed=crashed)
    return _WHOLE[name]
