"""The NTSC line services (white flag, closed captions, video ID): the numpy restatement of the
build-defined rule (csrc/lines.hip is held to it exactly), writers of ideal
rows with known answers, and captures that carry the three lines through the whole RF chain
(test infrastructure, modelled on tests/vbi_cases.py whose START, BASE, TAIL and Read it reuses).

The rule is integer arithmetic on the uint16 pixels p[0..909] of one .tbc row of a field: row 10
the white flag, row 19 the video ID, row 20 the captions (.tbc row r is line location r + 1).
Pixels 0 and 1 (the burst flag pixels) are never read.  A record is a dict with the members of
ldg_line_services (include/ldgpu.h).

``LineRF`` is a ``DamagedRF`` that draws the three lines of chosen (frame, field)s into the
composite signal; ``CASES`` is the table of captures read once each at damage.START['NTSC'] (field 1
of capture frame 0), with what the restatement makes of the oracle's dspicture (``expect``, asserted
on the CPU by test_lines_ref.py together with the robustness condition).  ``build_whole`` is the
capture for the decode loop, ``whole_expect`` what its fields carry.  test_lines_gpu.py holds the kernel, GPUDecoder and the tools to both.
"""
import numpy as np

import damage as D
from damage import BASE, START, TAIL, DamagedRF, Read  # noqa: F401
from ldgpu.synth import NTSC, SynthRF

W = 910
ROWS = 21                                  # rows a field needs
ROW_WHITE, ROW_VID, ROW_CC = 10, 19, 20
ABSENT, OK, CHECK, FRAME = 0, 1, 2, 3      # LDG_LINE_*


def level(ire):
    """The .tbc value of an IRE level: 1024 + (IRE + 40) * 358.4."""
    return 1024 + (ire + 40) * 358.4


T25, T35, T50 = 24320, 27904, 33280
assert (T25, T35, T50) == (level(25), level(35), level(50))
NO_FIELD = dict(white_count=-1, white_flag=0, cc_state=ABSENT, cc_runin=0, cc_x=-1, cc=(0, 0), vid_state=ABSENT,
                vid_x=-1, vid_bits=0)


# ---- helpers of the rule ------------------------------------------------------------------------
def first_rise(p, T, lo, hi, q):
    """The smallest x in [lo, hi) with p[x] > T and p[x - q .. x - 1] all <= T, or -1."""
    for x in range(lo, hi):
        if p[x] > T and not (p[x - q:x] > T).any():
            return x
    return -1


def cell(p, c, T):
    """A cell at centre c reads 1 iff the nine pixels about it sum above 9 T (a tie reads 0)."""
    return int(int(p[c - 4:c + 5].sum()) > 9 * T)


def odd_parity(b):
    return bin(b & 0xFF).count('1') & 1 == 1


def with_parity(c):
    """The 7-bit character c with its odd-parity bit in bit 7."""
    c &= 0x7F
    return c if odd_parity(c) else c | 0x80


def vid_crc_reg(bits, reg=0x3F):
    """The CRC register (x^6 + x + 1, preset to ones) after the given bits, first bit first."""
    for bit in bits:
        fb = ((reg >> 5) & 1) ^ bit
        reg = ((reg << 1) & 0x3F) ^ (3 if fb else 0)
    return reg


def vid_word(data):
    """The 20 bits (14 data bits, then the 6 CRC bits that leave the register at zero)."""
    data &= 0x3FFF
    reg = vid_crc_reg([(data >> (13 - i)) & 1 for i in range(14)])
    return (data << 6) | reg


def bits_of(word, n):
    return [(word >> (n - 1 - i)) & 1 for i in range(n)]


# ---- the rule -----------------------------------------------------------------------------------
def white_flag(p):
    p = np.asarray(p, dtype=np.int64)
    count = int((p[100:780] > T50).sum())
    return dict(white_count=count, white_flag=int(2 * count > 680))


def captions(p):
    p = np.asarray(p, dtype=np.int64)
    xs = first_rise(p, T25, 270, 410, 40)
    if xs < 0:
        return dict(cc_state=ABSENT, cc_runin=0, cc_x=-1, cc=(0, 0))
    b = p > T25
    # (pixels 0 and 1 are never read: an edge needs x - 1 >= 2)
    runin = sum(1 for x in range(max(xs - 279, 3), xs - 40) if b[x] and not b[x - 1])
    bits = [cell(p, (32 * xs + (3 + 2 * i) * 455) >> 5, T25) for i in range(16)]
    b0 = sum(v << i for i, v in enumerate(bits[:8]))
    b1 = sum(v << i for i, v in enumerate(bits[8:]))
    if not 6 <= runin <= 8:
        state = FRAME
    else:
        state = OK if odd_parity(b0) and odd_parity(b1) else CHECK
    return dict(cc_state=state, cc_runin=runin, cc_x=xs, cc=(b0, b1))


def video_id(p):
    p = np.asarray(p, dtype=np.int64)
    xr = first_rise(p, T35, 60, 160, 20)
    if xr < 0:
        return dict(vid_state=ABSENT, vid_x=-1, vid_bits=0)
    cells = [cell(p, xr + 16 + 32 * j, T35) for j in range(22)]
    word = 0
    for v in cells[2:]:
        word = (word << 1) | v
    if cells[:2] != [1, 0]:
        state = FRAME
    else:
        state = OK if vid_crc_reg(cells[2:]) == 0 else CHECK
    return dict(vid_state=state, vid_x=xr, vid_bits=word)


def decode_field(rows):
    """The record of a field from its rows [>= 21, 910]; None or fewer rows: no such field."""
    if rows is None or len(rows) < ROWS:
        return dict(NO_FIELD)
    return dict(**white_flag(rows[ROW_WHITE]), **captions(rows[ROW_CC]), **video_id(rows[ROW_VID]))


def decode_frames(frames):
    """[n][2] records of packed frames [n, 525, 910]: frame row y is row y >> 1 of the field of parity y & 1."""
    fr = np.asarray(frames).reshape(-1, 525, W)
    return [[decode_field(f[p::2][:ROWS]) for p in (0, 1)] for f in fr]


def json_record(rec):
    """The record as GPUDecoder writes it into a field's 'lineServices'."""
    return {'white': bool(rec['white_flag']), 'whiteCount': int(rec['white_count']),
            'cc': [int(rec['cc'][0]), int(rec['cc'][1])] if rec['cc_state'] != ABSENT else None,
            'ccState': int(rec['cc_state']),
            'videoId': int(rec['vid_bits']) >> 6 if rec['vid_state'] == OK else None,
            'videoIdBits': int(rec['vid_bits']), 'videoIdState': int(rec['vid_state'])}


# ---- ideal rows (pixel level, hard edges) -------------------------------------------------------
L0, L50, L70, L100 = int(level(0)), int(level(50)), int(level(70)), int(level(100))


def blank_row():
    return np.full(W, L0, dtype=np.uint16)


def ideal_white(count, hi=L100):
    """A row with exactly `count` pixels of [100, 780) above 50 IRE."""
    p = blank_row()
    p[100:100 + count] = hi
    return p


def ideal_cc(xs, b0, b1, rises=7, hi=L50):
    """A caption row whose start bit rises at xs: `rises` pulses of 10 pixels, 20 apart, the last
    ending 50 pixels before xs; then the start bit and the 16 bits in cells of 910 / 32 pixels."""
    p = blank_row()
    for k in range(rises):
        a = xs - 60 - 20 * k
        p[max(a, 0):max(a + 10, 0)] = hi
    bits = [1] + [(b0 >> i) & 1 for i in range(8)] + [(b1 >> i) & 1 for i in range(8)]
    for x in range(xs, W):
        c = ((x - xs) * 32) // W
        if c < len(bits) and bits[c]:
            p[x] = hi
    return p


def cc_centre(xs, i):
    return (32 * xs + (3 + 2 * i) * 455) >> 5


def ideal_vid(xr, word, ref=(1, 0), hi=L70):
    """A video ID row whose reference rises at xr: 22 cells of 32 pixels."""
    p = blank_row()
    for j, v in enumerate(list(ref) + bits_of(word, 20)):
        if v:
            p[xr + 32 * j:xr + 32 * j + 32] = hi
    return p


def ideal_field(white=None, cc=None, vid=None):
    """21 blank rows with the given service rows."""
    rows = np.tile(blank_row(), (ROWS, 1))
    for r, p in ((ROW_WHITE, white), (ROW_CC, cc), (ROW_VID, vid)):
        if p is not None:
            rows[r] = p
    return rows


def pack_frames(fields):
    """Fields [(top rows, bottom rows), ...] as packed frames [n, 525, 910] (the rest zero)."""
    out = np.zeros((len(fields), 525, W), dtype=np.uint16)
    for f, (top, bot) in enumerate(fields):
        out[f, 0:2 * len(top):2] = top
        out[f, 1:2 * len(bot):2] = bot
    return out


# ---- captures -----------------------------------------------------------------------------------
# the 0-based frame line of .tbc row r: r + 1 in field 0, r + 264 in field 1 (the Philips code lines
# 16..18 / 279..281 are rows 15..17)
FRAME_LINE = {0: {'white': ROW_WHITE + 1, 'vid': ROW_VID + 1, 'cc': ROW_CC + 1},
              1: {'white': ROW_WHITE + 264, 'vid': ROW_VID + 264, 'cc': ROW_CC + 264}}
KINDS = {'white': ('ire',),
         'cc': ('bytes', 'shift', 'swing', 'flat_cell', 'no_runin'),
         'vid': ('word', 'ref', 'shift', 'swing', 'flat_cell')}
H = NTSC['line_us']
CC_CELL = H / 32
VID_CELL = 8 / (NTSC['fsc'] / 1e6)


class LineRF(DamagedRF):
    """DamagedRF that draws service lines.  lines: {(k, field, service): spec} for frame k, field
    0 / 1, service 'white' / 'cc' / 'vid'.  The line's span from 9.4 us to H - 1.5 us is first set to
    0 IRE, then:
      white  100 IRE (ire=...) from 10 to 60 us;
      cc     bytes=(b0, b1) as sent (parity bit included): from 10.0 us seven cycles of
             25 - 25 cos(2 pi (tau - 10) / c), c = H / 32, then 19 hard-edged cells of width c:
             0, 0, 1 and the 16 bits LSB first, at 50 IRE (swing=...); shift=d: the train d us late;
             flat_cell=(k, ire): cell k of the 19 held at that level; no_runin: the cycles left out;
      vid    word=20 bits (vid_word(data)): from 11.2 us 22 hard-edged cells of 8 / fsc us: ref
             (default (1, 0)), the 14 data bits, the 6 CRC bits, at 70 IRE (swing=...); shift,
             flat_cell=(k, ire) of the 22 likewise.
    An empty spec leaves the line at 0 IRE.  The parent's `edits` apply afterwards, its RF
    `dropouts` to the modulated carrier."""

    def __init__(self, lines=None, **kw):
        super().__init__(**kw)
        self.lines = {}
        for (k, fld, svc), spec in (lines or {}).items():
            assert set(spec) <= set(KINDS[svc]), (svc, spec)
            self.lines[(int(k), int(fld), svc)] = dict(spec)

    def _ire(self, n):
        ire = SynthRF._ire(self, n)
        if self.lines:
            self._service_lines(n, ire)
        return self._apply_edits(n, ire)

    def _service_lines(self, n, ire):
        L = self.p['lines']
        la = n / self.spl + self.t0_lines
        fl = np.floor(la).astype(np.int64)              # absolute line, ascending
        for (k, fld, svc), spec in self.lines.items():
            line = k * L + FRAME_LINE[fld][svc]
            i0, i1 = np.searchsorted(fl, line, 'left'), np.searchsorted(fl, line, 'right')
            if i0 == i1:
                continue
            tau = (la[i0:i1] - fl[i0:i1]) * H
            seg = ire[i0:i1]
            seg[(tau >= 9.4) & (tau < H - 1.5)] = 0.0
            if svc == 'white':
                if 'ire' in spec:
                    seg[(tau >= 10.0) & (tau < 60.0)] = spec['ire']
            elif svc == 'cc' and 'bytes' in spec:
                b0, b1 = spec['bytes']
                t = tau - 10.0 - spec.get('shift', 0.0)
                a = float(spec.get('swing', 50.0))
                if not spec.get('no_runin'):
                    m = (t >= 0) & (t < 7 * CC_CELL)
                    seg[m] = (a / 2) * (1 - np.cos(2 * np.pi * t[m] / CC_CELL))
                bits = np.array([0, 0, 1] + [(b0 >> i) & 1 for i in range(8)] + [(b1 >> i) & 1 for i in range(8)])
                self._cells(seg, t - 7 * CC_CELL, CC_CELL, bits, a, spec)
            elif svc == 'vid' and 'word' in spec:
                t = tau - 11.2 - spec.get('shift', 0.0)
                bits = np.array(list(spec.get('ref', (1, 0))) + bits_of(spec['word'], 20))
                self._cells(seg, t, VID_CELL, bits, float(spec.get('swing', 70.0)), spec)

    @staticmethod
    def _cells(seg, t, width, bits, a, spec):
        c = np.floor(t / width).astype(np.int64)
        inside = (c >= 0) & (c < len(bits))
        cc = c[inside]
        out = np.where(bits[cc] == 1, a, 0.0)
        if 'flat_cell' in spec:
            k, lvl = spec['flat_cell']
            out[cc == k] = lvl
        seg[inside] = out


def robust(rows, seed=20240611):
    """The robustness condition: the same record on the rows + 1, - 1 and with seeded noise in
    {-1, 0, 1} (the GPU's .tbc is held to +-1 LSB of the oracle's)."""
    rows = np.asarray(rows, dtype=np.int64)
    base = decode_field(rows)
    noise = np.random.default_rng(seed).integers(-1, 2, rows.shape)
    return all(decode_field(np.clip(rows + d, 0, 65535)) == base for d in (1, -1, noise))


class LRead(Read):
    """damage.Read with what the rule makes of the oracle's dspicture."""

    def rows(self):
        f = self.field
        return np.asarray(f.dspicture).reshape(f.linecount, W)

    def facts(self):
        d = dict(outcome=self.outcome)
        if self.outcome == 'valid':
            rows = self.rows()
            d.update(record=decode_field(rows), robust=robust(rows[:ROWS]))
        return d


CASES = {}
_CAP, _FACTS = {}, {}


def generator(c):
    return LineRF(system='NTSC', lines=c['lines'], edits=c['edits'], dropouts=c['dropouts'], **BASE)


def build(case):
    """The capture of a case: u8 samples 0 .. read start + TAIL."""
    c = CASES[case] if isinstance(case, str) else case
    g = generator(c)
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


def facts(case):
    if case not in _FACTS:
        c = CASES[case]
        _FACTS[case] = LRead('NTSC', capture(case), c['reads'][0]).facts()
    return _FACTS[case]


def E(white=None, cc=None, cc_state=None, vid=None, vid_state=None, vid_bits=None, runin=None):
    """What the rule makes of the oracle's read: white flag; cc bytes and state; video ID data
    (the 14 bits of an OK word), state and, where it matters, the 20 bits read."""
    return {k: v for k, v in dict(white=white, cc=cc, cc_state=cc_state, vid=vid, vid_state=vid_state,
                                  vid_bits=vid_bits, runin=runin).items() if v is not None}


def matches(rec, e):
    """The claims of an E against a record, as a list of the members that differ."""
    got = dict(white=bool(rec['white_flag']), cc=tuple(rec['cc']), cc_state=rec['cc_state'],
               vid=rec['vid_bits'] >> 6, vid_state=rec['vid_state'], vid_bits=rec['vid_bits'], runin=rec['cc_runin'])
    return [(k, got[k], v) for k, v in e.items() if got[k] != (tuple(v) if k == 'cc' else v)]


def _c(expect, white=None, cc=None, vid=None, **kw):
    """A case whose three lines lie in field 1 of frame 0 (the field the read at START decodes)."""
    lines = {}
    for svc, spec in (('white', white), ('cc', cc), ('vid', vid)):
        if spec is not None:
            lines[(0, 1, svc)] = spec
    return D._case('NTSC', expect=expect, lines=lines, **kw)


AY = (0xC1, 0x79)                      # 'A', 'y' with their parity bits
VID = vid_word(0x152E)


def _table():
    T = {}
    # a plain SynthRF capture: row 10 blank, rows 19 and 20 picture (bars): no white flag, no captions
    # (the bars never stay 40 pixels under 25 IRE before a rise in the window), no valid video ID
    T['plain'] = D._case('NTSC', expect=E(white=False, cc_state=ABSENT), lines={})
    # the three lines as drawn, nothing damaged
    T['clean'] = _c(E(white=True, cc=AY, cc_state=OK, runin=7, vid=0x152E, vid_state=OK),
                    white=dict(ire=100.0), cc=dict(bytes=AY), vid=dict(word=VID))
    # the lines blanked: every service absent, and the flag's other value on a drawn line
    T['blank'] = _c(E(white=False, cc_state=ABSENT, vid_state=ABSENT), white={}, cc={}, vid={})
    # a white line at 45 IRE stays under the 50 IRE threshold; a wrong parity bit; a wrong CRC bit
    T['check'] = _c(E(white=False, cc=(0x41, 0x79), cc_state=CHECK, vid_state=CHECK, vid_bits=VID ^ 1),
                    white=dict(ire=45.0), cc=dict(bytes=(0x41, 0x79)), vid=dict(word=VID ^ 1))
    # the run-in removed: no rises before the start bit; the reference swapped: the first rise is cell 1
    # and the cells read from there begin 1, d0
    T['frame'] = _c(E(white=True, cc=AY, cc_state=FRAME, runin=0, vid_state=FRAME),
                    white=dict(ire=100.0), cc=dict(bytes=AY, no_runin=True),
                    vid=dict(word=vid_word(0x3FFF), ref=(0, 1)))
    # the trains 1.5 us early and 1.5 us late (21 pixels): inside both search windows
    T['early'] = _c(E(cc=AY, cc_state=OK, vid=0x152E, vid_state=OK),
                    cc=dict(bytes=AY, shift=-1.5), vid=dict(word=VID, shift=-1.5))
    T['late'] = _c(E(cc=AY, cc_state=OK, vid=0x152E, vid_state=OK),
                   cc=dict(bytes=AY, shift=1.5), vid=dict(word=VID, shift=1.5))
    # 8 us late: the caption start bit leaves [270, 410) (absent); the video ID's reference leaves [60, 160)
    T['far'] = _c(E(cc_state=ABSENT, vid_state=ABSENT),
                  cc=dict(bytes=AY, shift=8.0), vid=dict(word=VID, shift=8.0))
    # the swing reduced: 35 IRE captions still cross 25 IRE, a 20 IRE video ID never crosses 35 IRE
    # (at 30 IRE the overshoot of the reference's edge does)
    T['swing'] = _c(E(cc=AY, cc_state=OK, vid_state=ABSENT),
                    cc=dict(bytes=AY, swing=35.0), vid=dict(word=VID, swing=20.0))
    # one cell held flat: caption cell 4 (bit 1 of byte 0, a zero of 0xC1) at 50 IRE: 0xC3, even parity;
    # video ID cell 3 (the second data bit, a one of 0x152E) at 0 IRE: the CRC fails
    T['flat_cell'] = _c(E(cc=(0xC3, 0x79), cc_state=CHECK, vid_state=CHECK, vid_bits=VID ^ (1 << 18)),
                        cc=dict(bytes=AY, flat_cell=(4, 50.0)), vid=dict(word=VID, flat_cell=(3, 0.0)))
    # an edit to 0 IRE across byte 1 of the caption line (from 46 us: it reads 0, even parity), and
    # an RF dropout of 30 us across the video ID line (frame line 283 starts at sample 465226): the
    # reference is found, the noise after it is not 1, 0
    T['edit'] = _c(E(white=True, cc=(0xC1, 0x00), cc_state=CHECK, vid_state=FRAME),
                   white=dict(ire=100.0), cc=dict(bytes=AY), vid=dict(word=VID),
                   edits=[(FRAME_LINE[1]['cc'] + 46.0 / H, 17.0 / H, 0.0)], dropouts=((465826, 1200),))
    return T


CASES.update(_table())


# ---- a whole capture for the decode loop --------------------------------------------------------
# Capture frame k starts at line 525 k; the capture starts at line 100 of frame 0, so the decode's
# frame i is made of the two fields of capture frame i + 1.
WHOLE_SECONDS = 0.3
WHOLE_TEXT = 'LINE SERVICES ON GPU'


def whole_sequence(nframes=12):
    """Per capture frame k and field: (white, (b0, b1), video ID data).  White flags in a 3:2
    cadence (a film frame starts at fields 0, 2, 5, 7 of every ten); the text two characters a
    field; the video ID changes once, at frame 5."""
    seq = {}
    text = (WHOLE_TEXT * 8).encode()
    for k in range(nframes):
        for fld in (0, 1):
            i = 2 * k + fld
            seq[(k, fld)] = (i % 10 in (0, 2, 5, 7), (with_parity(text[2 * i]), with_parity(text[2 * i + 1])),
                             0x152E if k < 5 else 0x2A51)
    return seq


def whole_lines():
    lines = {}
    for (k, fld), (white, cc, vid) in whole_sequence().items():
        lines[(k, fld, 'white')] = dict(ire=100.0) if white else {}
        lines[(k, fld, 'cc')] = dict(bytes=cc)
        lines[(k, fld, 'vid')] = dict(word=vid_word(vid))
    return lines


_WHOLE = {}


def build_whole():
    if 'data' not in _WHOLE:
        g = LineRF(system='NTSC', lines=whole_lines(), **BASE)
        left, parts = int(40e6 * WHOLE_SECONDS), []
        while left > 0:
            n = min(1 << 22, left)
            parts.append(SynthRF.quantise(g.generate(n), 'u8'))
            left -= n
        _WHOLE['data'] = np.concatenate(parts).tobytes()
    return _WHOLE['data']


def whole_expect(k, fld):
    """The 'lineServices' record of capture frame k's field."""
    white, cc, vid = whole_sequence()[(k, fld)]
    return {'white': white, 'cc': list(cc), 'ccState': OK, 'videoId': vid, 'videoIdBits': vid_word(vid),
            'videoIdState': OK}
