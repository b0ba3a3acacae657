"""EFM data sectors on the GPU (csrc/efmsec.hip; BUILD-DEFINED): the
decoded EFM stream's bytes before concealment, with per-byte erasures, to the 2048 user bytes of
each CD-ROM mode 1 sector -- the walk over a .efm file in chunks with the stage attached to the
EFM decode, the stage on its own over bytes, and the summary.
"""
import numpy as np

from . import efmdec

COUNTERS = ('sectors', 'candidates', 'confirmed', 'coasted', 'breaks', 'good', 'corrected', 'bad', 'other', 'p_fixed',
            'q_fixed', 'erased_bytes')
STATUS = ('good', 'corrected', 'bad', 'other')               # LDG_EFMSEC_*
ARRAYS = ('data', 'records', 'starts')
PARITY_ARRAYS = ('sectors', 'bytes', 'erased')
MAX_BAD_LISTED = 1000


def _collect(ctx, info, parts, tot):
    for k in COUNTERS:
        tot[k] += info[k]
    for k in parts:
        parts[k].append(ctx.efmsec_read(k, info['bytes'] if k in ('bytes', 'erased') else info['sectors']))


def _result(parts, tot):
    res = {k: np.concatenate(v) for k, v in parts.items()}
    res['counters'] = tot
    return res


def decode_bytes(ctx, data, erased, chunk_bytes=None, keep=False):
    """The stage on its own: the bytes `data` and their erasure flags (uint8 arrays) -> dict with
    data uint8[n, 2048], records (native.EFMSEC_REC), starts int64[n] and the counters; keep:
    also the whole sectors.  The result does not depend on chunk_bytes."""
    ctx.efmsec_reset()
    n = int(data.size)
    step = n if not chunk_bytes else max(int(chunk_bytes), 1)
    parts = {k: [] for k in ARRAYS + (('sectors',) if keep else ())}
    tot = dict.fromkeys(COUNTERS, 0)
    at = 0
    while True:
        b = min(at + step, n)
        _collect(ctx, ctx.efmsec_feed(np.asarray(data[at:b]), np.asarray(erased[at:b]), final=b >= n), parts, tot)
        at = b
        if at >= n:
            break
    return _result(parts, tot)


def decode(ctx, rl, chunk_bytes=None, table=None, keep=False):
    """The run lengths `rl` through the EFM decode with the sector stage attached -> (the
    decode's result as efmdec.decode gives it, the stage's as decode_bytes gives it; keep: also
    the parity arrays of both).  Detaches the stage again."""
    ctx.efmsec_enable(True)
    try:
        parts = {k: [] for k in ARRAYS + (PARITY_ARRAYS if keep else ())}
        tot = dict.fromkeys(COUNTERS, 0)
        pcm = efmdec.decode(ctx, rl, chunk_bytes, table, keep,
                            after_feed=lambda: _collect(ctx, ctx.efmsec_last_info(), parts, tot))
    finally:
        ctx.efmsec_enable(False)
    return pcm, _result(parts, tot)


def bcd(v):
    return (int(v) >> 4) * 10 + (int(v) & 15)


def address(rec):
    """A record's header as a sector count (75 a second), or None where it is no BCD."""
    m, s, f = int(rec['minute']), int(rec['second']), int(rec['frame'])
    if any((v >> 4) > 9 or (v & 15) > 9 for v in (m, s, f)):
        return None
    return (bcd(m) * 60 + bcd(s)) * 75 + bcd(f)


def summary(res):
    """The counters, the first and last address [min, sec, frame] among the good and corrected
    sectors, the discontinuities between consecutive such sectors (an address that is not the one
    before plus the sectors between them), and the first 1000 bad sectors."""
    rec, starts = res['records'], res['starts']
    summ = dict(res['counters'])
    ok = np.nonzero(rec['status'] <= 1)[0]
    adr = [(int(i), address(rec[i])) for i in ok]
    adr = [(i, a) for i, a in adr if a is not None]
    summ['first_address'] = [bcd(rec[adr[0][0]][k]) for k in ('minute', 'second', 'frame')] if adr else None
    summ['last_address'] = [bcd(rec[adr[-1][0]][k]) for k in ('minute', 'second', 'frame')] if adr else None
    summ['address_discontinuities'] = sum(1 for (i, a), (j, b) in zip(adr[:-1], adr[1:]) if b - a != j - i)
    bad = np.nonzero(rec['status'] >= 2)[0][:MAX_BAD_LISTED]
    summ['bad_sectors'] = [{'index': int(i), 'start_byte': int(starts[i]), 'status': STATUS[int(rec['status'][i])],
                            'erased': int(rec['erased'][i])} for i in bad]
    return summ


def decode_file(ctx, path, outbase, chunk_bytes=1 << 24, table=None, stats=False):
    """`path`'s run lengths into <outbase>.efm.pcm and .efm.pcm.json as efmdec.decode_file writes
    them, and into <outbase>.efm.data (2048 bytes a sector, grid order) and
    <outbase>.efm.data.json; returns (the PCM summary, the data summary)."""
    import json
    ctx.efmsec_enable(True)
    try:
        parts = {k: [] for k in ARRAYS}
        tot = dict.fromkeys(COUNTERS, 0)
        kernels = {}
        psumm = efmdec.decode_file(ctx, path, outbase, chunk_bytes, table, stats,
                                   after_feed=lambda: _collect(ctx, ctx.efmsec_last_info(), parts, tot), all_kernels=kernels)
    finally:
        ctx.efmsec_enable(False)
    res = _result(parts, tot)
    with open(outbase + '.efm.data', 'wb') as fh:
        fh.write(res['data'].tobytes())
    summ = summary(res)
    if stats:
        summ['kernels_ms'] = {k: v for k, v in kernels.items() if k.startswith('efmsec_')}
    with open(outbase + '.efm.data.json', 'w') as fh:
        json.dump(summ, fh, indent=1)
    return psumm, summ
