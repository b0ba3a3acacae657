"""Host side of the disc stacker: which frames of which sources make
an output frame, the sources' dropout runs in the library's array layout, and the runs the
stack could not fill.  Pure Python and numpy: no library, no GPU."""
import numpy as np

MAX_LINES = 320                   # rows of a field's run arrays (native.MAX_LINES)
MAX_PER_LINE = 8                  # LDG_MAX_DROPOUTS_PER_LINE
MAX_SOURCES = 16                  # LDG_STACK_MAX_SOURCES
OUTW = {'NTSC': 910, 'PAL': 1135}
FRAME_LINES = {'NTSC': 525, 'PAL': 625}
MODES = ('median', 'mean', 'smart-mean')
DEFAULT_THRESHOLD = 3840          # 15 on an 8-bit scale


class StackError(ValueError):
    pass


def frame_fields(record):
    """The records of the frame's top and bottom fields: the last valid one of each parity
    (GPUDecoder.readframe's choice), or None where the frame has no valid field of one."""
    top = bottom = None
    for x in record.get('fields', ()):
        if not x.get('valid'):
            continue
        if x.get('istop'):
            top = x
        else:
            bottom = x
    return None if top is None or bottom is None else (top, bottom)


def empty_runs():
    return (np.zeros((2, MAX_LINES, MAX_PER_LINE, 2), dtype=np.int16), np.zeros((2, MAX_LINES), dtype=np.int32))


def frame_runs(record, system, where=''):
    """(runs int16 [2, MAX_LINES, 8, 2], counts int32 [2, MAX_LINES], (top, bottom line
    counts), whether both fields carry a 'dropouts' key) of one frame record; None for a
    record without a valid field of either parity (the source is not present for the frame).
    A field without the key has no runs.  A ninth or later run of a row extends the eighth's
    endx (detection's rule 7).  A run outside the arrays or the row raises StackError."""
    ff = frame_fields(record)
    if ff is None:
        return None
    W = OUTW[system]
    runs, counts = empty_runs()
    keyed = True
    for p, x in enumerate(ff):
        if 'dropouts' not in x:
            keyed = False
            continue
        for run in x['dropouts']:
            row, sx, ex = (int(v) for v in run)
            if not 0 <= row < MAX_LINES:
                raise StackError('%sdropout row %d outside [0, %d)' % (where, row, MAX_LINES))
            if not 0 <= sx < ex <= W:
                raise StackError('%sdropout run [%d, %d) of row %d is not within 0 <= startx < endx <= %d'
                                 % (where, sx, ex, row, W))
            k = counts[p, row]
            if k < MAX_PER_LINE:
                runs[p, row, k] = (sx, ex)
                counts[p, row] = k + 1
            elif ex > runs[p, row, k - 1, 1]:
                runs[p, row, k - 1, 1] = ex
    return runs, counts, (int(ff[0]['linecount']), int(ff[1]['linecount'])), keyed


def align(metas, by_index=False, start=None, length=None, min_sources=1):
    """Which frame of each source makes each output frame.  metas: per source the list of
    frame records.  A frame's key is its record's vbi framenr (by_index: its position in the
    file); a frame without a key, or whose key an earlier frame of the same source has, is
    left out of that source.  The output frames are the ascending union of the keys at least
    min_sources sources have, cut to the keys in [start, start + length) (start None: from
    the lowest key; length None: to the end).
    Returns ([(key, [frame index in source s, or None])], [{'no_key': n, 'repeated': n} per
    source])."""
    maps, skipped = [], []
    for meta in metas:
        m, sk = {}, {'no_key': 0, 'repeated': 0}
        for i, rec in enumerate(meta):
            key = i if by_index else (rec.get('vbi') or {}).get('framenr')
            if key is None:
                sk['no_key'] += 1
            elif key in m:
                sk['repeated'] += 1
            else:
                m[key] = i
        maps.append(m)
        skipped.append(sk)
    need = max(1, int(min_sources))
    keys = sorted(k for k in set().union(*maps) if sum(k in m for m in maps) >= need) if maps else []
    if keys and (start is not None or length is not None):
        lo = keys[0] if start is None else start
        keys = [k for k in keys if k >= lo and (length is None or k < lo + length)]
    return [(k, [m.get(k) for m in maps]) for k in keys], skipped


def _union(runs, count, W):
    """One source's runs of a row as disjoint ascending [a, b) (the device's reading: a count
    above 8 is 8, the row's bounds clip)."""
    iv = sorted((max(0, int(a)), min(W, int(b))) for a, b in runs[:min(int(count), MAX_PER_LINE)])
    out = []
    for a, b in iv:
        if a >= b:
            continue
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def residual(runs, counts, W):
    """The pixels every present source lost: runs int16 [S, 2, MAX_LINES, 8, 2] and counts
    int32 [S, 2, MAX_LINES] of the S present sources -> (runs [2, MAX_LINES, 8, 2], counts
    [2, MAX_LINES]), per (parity, row) the intersection over the sources of each source's
    union of runs, merged, a ninth or later run extending the eighth."""
    runs, counts = np.asarray(runs), np.asarray(counts)
    out_r, out_c = empty_runs()
    for p, r in zip(*np.nonzero((counts > 0).all(axis=0))):
        cur = _union(runs[0, p, r], counts[0, p, r], W)
        for s in range(1, runs.shape[0]):
            other, nxt = _union(runs[s, p, r], counts[s, p, r], W), []
            for a, b in cur:
                for c, d in other:
                    lo, hi = max(a, c), min(b, d)
                    if lo < hi:
                        nxt.append([lo, hi])
            cur = nxt
            if not cur:
                break
        for a, b in cur:
            k = out_c[p, r]
            if k and a <= out_r[p, r, k - 1, 1]:
                out_r[p, r, k - 1, 1] = max(out_r[p, r, k - 1, 1], b)
            elif k < MAX_PER_LINE:
                out_r[p, r, k] = (a, b)
                out_c[p, r] = k + 1
            else:
                out_r[p, r, k - 1, 1] = max(out_r[p, r, k - 1, 1], b)
    return out_r, out_c


def runs_list(runs, counts, p):
    """[[row, startx, endx], ...] of parity p in (row, startx) order: a record's 'dropouts'."""
    return [[int(r), int(runs[p, r, k, 0]), int(runs[p, r, k, 1])]
            for r in np.flatnonzero(counts[p] > 0) for k in range(min(int(counts[p, r]), MAX_PER_LINE))]


def output_record(record, index, key, sources, res_runs, res_counts):
    """base's record as the output frame's: its index, the two fields used with the
    residual dropouts, and where the frame came from."""
    out = dict(record)
    out['frame'] = index
    top, bottom = frame_fields(record)
    out['fields'] = [dict(x, dropouts=runs_list(res_runs, res_counts, 0 if x is top else 1))
                     for x in record['fields'] if x is top or x is bottom]
    out['stack'] = {'framenr': key, 'sources': [int(s) for s in sources]}
    return out
