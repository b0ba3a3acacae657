"""numpy restatement of the dropout rules: detection per field row
from the demod channel and the final line locations, concealment on an assembled frame.
The GPU kernels (csrc/dropout.hip) are checked against this file; the rule itself is
build-defined (the snapshot the project follows has no dropout handling)."""
import math

import numpy as np

MAX_PER_LINE = 8                        # LDG_MAX_DROPOUTS_PER_LINE
LOFF = {'NTSC': 1, 'PAL': 3}            # final_lines: line l = row + LOFF
FIRST_ROW = {'NTSC': 21, 'PAL': 22}     # LDG_CONCEAL_FIRST_ROW
LINE_STEP = {'NTSC': 2, 'PAL': 4}       # field rows with the same chroma phase (and V-switch)
OUTW = {'NTSC': 910, 'PAL': 1135}
FRAME_LINES = {'NTSC': 525, 'PAL': 625}
SYS = {'NTSC': dict(ire0=8100000.0, hz_ire=1700000 / 140.0, vsync_ire=-40.0),
       'PAL': dict(ire0=7100000.0, hz_ire=800000 / 100.0, vsync_ire=-.3 * (100 / .7))}


def defaults(system):
    """ldg_dropout_defaults."""
    return dict(lo_ire=SYS[system]['vsync_ire'] - 50, hi_ire=150.0, merge_gap=80, min_flagged=3, pad=24, conceal=0)


def thresholds(system, opts):
    s = SYS[system]
    return s['ire0'] + s['hz_ire'] * opts['lo_ire'], s['ire0'] + s['hz_ire'] * opts['hi_ire']


def sample_runs(flagged, ib, ie, merge_gap=80, min_flagged=3, pad=24):
    """Steps 2-4: the padded, merged sample runs [a, b] (inclusive, absolute indices) of one
    row whose samples are [ib, ie); flagged[k] belongs to sample ib + k."""
    idx = np.flatnonzero(np.asarray(flagged, dtype=bool)) + ib
    raw = []
    for j in idx.tolist():
        if raw and j - raw[-1][1] <= merge_gap:
            raw[-1][1] = j
            raw[-1][2] += 1
        else:
            raw.append([j, j, 1])
    out = []
    for a, b, cnt in raw:
        if cnt < min_flagged:
            continue
        a, b = max(ib, a - pad), min(ie - 1, b + pad)
        if out and a <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(r) for r in out]


def pixel_runs(runs, begin, end, W):
    """Steps 5-7: sample runs -> [startx, endx) pixel runs of a W-pixel row."""
    sc = W / (end - begin)
    out = []
    for a, b in runs:
        sx = max(0, math.floor((a - begin) * sc))
        ex = min(W, math.ceil((b + 1 - begin) * sc))
        if out and sx <= out[-1][1]:
            out[-1][1] = max(out[-1][1], ex)
        elif len(out) < MAX_PER_LINE:
            out.append([sx, ex])
        else:
            out[-1][1] = max(out[-1][1], ex)
    return [tuple(r) for r in out]


def detect_row(demod, begin, end, W, lo_hz, hi_hz, merge_gap=80, min_flagged=3, pad=24):
    ib, ie = int(begin), int(end)
    d = demod[ib:ie]
    with np.errstate(invalid='ignore'):
        flagged = ~((lo_hz <= d) & (d <= hi_hz))
    return pixel_runs(sample_runs(flagged, ib, ie, merge_gap, min_flagged, pad), begin, end, W)


def detect_field(demod, linelocs, linecount, system, opts=None):
    """Every run of one valid field in (row, startx) order: [(row, startx, endx)].
    linelocs: the final line locations, indexed by line (line 0 first)."""
    o = dict(defaults(system), **(opts or {}))
    lo, hi = thresholds(system, o)
    out = []
    for r in range(linecount):
        l = r + LOFF[system]
        for sx, ex in detect_row(demod, float(linelocs[l]), float(linelocs[l + 1]), OUTW[system], lo, hi,
                                 o['merge_gap'], o['min_flagged'], o['pad']):
            out.append((r, sx, ex))
    return out


def conceal_source(r, sx, ex, runs_by_row, nrows, system, p=0):
    """The field row a run [sx, ex) of row r is copied from, or None.  runs_by_row: the
    field's {row: [(startx, endx)]}; nrows: min of the frame's two line counts; p: the
    field's parity (frame row = 2 * field row + p)."""
    d = LINE_STEP[system]
    for c in (r - d, r + d, r - 2 * d, r + 2 * d):
        if c < FIRST_ROW[system] or c >= nrows or 2 * c + p >= FRAME_LINES[system]:
            continue
        if any(cs < ex and sx < ce for cs, ce in runs_by_row.get(c, ())):
            continue
        return c
    return None


def conceal_frame(frame, top_runs, bottom_runs, lt, lb, system):
    """The concealed copy of one assembled frame (frame_lines x W uint16).  top_runs /
    bottom_runs: the fields' [(row, startx, endx)]; lt, lb: their line counts.
    Returns (frame, [(parity, row, startx, endx, source row or None)])."""
    W = OUTW[system]
    src = np.asarray(frame).reshape(FRAME_LINES[system], W)
    out = src.copy()
    nrows = min(lt, lb)
    log = []
    for p, runs in ((0, top_runs), (1, bottom_runs)):
        by_row = {}
        for r, sx, ex in runs:
            by_row.setdefault(r, []).append((sx, ex))
        for r, sx, ex in runs:
            if r < FIRST_ROW[system] or r >= nrows or 2 * r + p >= FRAME_LINES[system]:
                continue
            c = conceal_source(r, sx, ex, by_row, nrows, system, p)
            x0 = max(sx, 2) if system == 'NTSC' else sx      # pixels 0, 1: the burst flag pixels
            log.append((p, r, sx, ex, c))
            if c is not None and x0 < ex:
                out[2 * r + p, x0:ex] = src[2 * c + p, x0:ex]
    return out, log


# ---- the shared test capture and its oracle decode -------------------------------------
BASE = 2_500_000
SAMPLES_PER_LINE = {'NTSC': 40e6 * 227.5 / (315e6 / 88), 'PAL': 2560.0}


def capture_dropouts(system):
    """(first sample, count) of the synthesised dropouts: four of growing length (the last
    spans four rows), a cluster of nine short ones within a row's length (the per-row cap), and
    a pair LINE_STEP lines apart over the same pixels (the later one's first candidate is taken)."""
    step = int(round(LINE_STEP[system] * SAMPLES_PER_LINE[system]))
    return ((BASE, 100), (BASE + 170000, 200), (BASE + 340000, 1500), (BASE + 510000, 6000)) + \
        tuple((BASE + 680000 + 250 * k, 100) for k in range(9)) + \
        ((BASE + 850000, 400), (BASE + 850000 + step, 400))


_cache = {}


def capture(system):
    """The bytes of the shared 0.25 s u8 capture."""
    key = ('cap', system)
    if key not in _cache:
        from ldgpu.synth import make_capture
        _cache[key] = make_capture(int(40e6 * 0.25), 'u8', system=system, first_frame=200, seed=31,
                                   dropouts=capture_dropouts(system))
    return _cache[key]


def oracle_decode(system):
    """The oracle's decode of capture(system), once per process:
    {'frames', 'meta', 'fields': [per Field in read order: readsample, valid, linecount, istop,
    linelocs, origin (capture sample of demod index 0, before the filters' delay), runs (the
    restatement on the oracle's arrays), extents [(d0, dn, first, last flagged demod index)]]}."""
    key = ('dec', system)
    if key in _cache:
        return _cache[key]
    from oracle.capture import FMT_U8
    from oracle.framer import decode_capture
    lo, hi = thresholds(system, defaults(system))
    fields = []

    def on_field(f):
        rs = int(f.readsample)
        rec = {'readsample': rs, 'valid': bool(f.valid), 'origin': rs if rs > 1024 else 1024}
        if f.valid:
            dm = f.data[0]['demod']
            rec.update(linecount=int(f.linecount), istop=bool(f.istop),
                       linelocs=np.array(f.linelocs, dtype=np.float64),
                       runs=detect_field(dm, f.linelocs, f.linecount, system))
            ext = []
            for d0, dn in capture_dropouts(system):
                a, b = d0 - rec['origin'] - 500, d0 + dn - rec['origin'] + 1000
                l0 = float(f.linelocs[LOFF[system]])
                if dn < 1500 or a < l0 or b >= len(dm):
                    continue
                with np.errstate(invalid='ignore'):
                    fl = np.flatnonzero(~((lo <= dm[a:b]) & (dm[a:b] <= hi)))
                if fl.size:
                    ext.append((d0, dn, a + int(fl[0]), a + int(fl[-1])))
            rec['extents'] = ext
        fields.append(rec)

    frames, _, meta = decode_capture(capture(system), FMT_U8, system=system, on_field=on_field)
    _cache[key] = {'frames': frames, 'meta': meta, 'fields': fields}
    return _cache[key]
