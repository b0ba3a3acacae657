"""EFM run lengths (a .efm file) to 44.1 kHz PCM on the GPU (csrc/efmdec.hip; BUILD-DEFINED,
DESIGN.md section 7d): the code table, the walk over the file in chunks, the subcode Q
decode (host, numpy) and the summary.
"""
import os

import numpy as np

SYM_S0, SYM_S1, SYM_BAD = 0x100, 0x101, 0xFFFF
S0_BITS, S1_BITS = '00100000000001', '00000000010010'      # the two subcode sync words
# The table is data taken from the snapshot this project follows (its attic/efm-map), and
# tests/golden/ is the only place this repository may hold such data: so the product reads
# the fixture, relative to the repository root, and --efm-table names another copy.
DEFAULT_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                             'tests', 'golden', 'efm_map.txt')
COUNTERS = ('frames', 'samples', 'candidates', 'confirmed', 'coasted', 'breaks', 'bad_symbols', 'c1_pass', 'c1_fixed',
            'c1_erased', 'c2_pass', 'c2_fixed', 'c2_erasure_solved', 'c2_failed', 'c2_unsolved', 'flagged', 'averaged',
            'muted')
PARITY_ARRAYS = ('starts', 'f3', 'c1', 'c1_flags', 'c2', 'c2_flags')


def load_table(path=None):
    """The 256 code words of 14 channel bits (value 0 first; first channel bit = MSB) as ints."""
    path = DEFAULT_TABLE if path is None else path
    with open(path) as fh:
        words = [ln.strip() for ln in fh if ln.strip() and not ln.startswith('#')]
    if len(words) != 256 or any(len(w) != 14 or set(w) - set('01') for w in words):
        raise ValueError('%s: expected 256 lines of 14 channel bits' % path)
    table = [int(w, 2) for w in words]
    if len(set(table + [int(S0_BITS, 2), int(S1_BITS, 2)])) != 258:
        raise ValueError('%s: the code words and the two subcode syncs are not distinct' % path)
    return table


def inverse_table(table):
    """uint16[16384]: 0..255 a value, 0x100 / 0x101 S0 / S1, 0xFFFF no code word."""
    inv = np.full(1 << 14, SYM_BAD, dtype=np.uint16)
    inv[np.asarray(table)] = np.arange(256, dtype=np.uint16)
    inv[int(S0_BITS, 2)] = SYM_S0
    inv[int(S1_BITS, 2)] = SYM_S1
    return inv


def decode(ctx, rl, chunk_bytes=None, table=None, keep=False, after_feed=None):
    """The run lengths `rl` (uint8 array, e.g. a np.memmap) -> dict with pcm int16[n, 2], flags
    uint8[n, 2], subcode uint16[frames] and the counters; keep: also the parity arrays.
    ctx: a native.Context.  The result does not depend on chunk_bytes.  after_feed: called after
    every feed (ldgpu.efmsec collects the sector stage's output there)."""
    ctx.efmdec_set_table(inverse_table(load_table(table)))
    n = int(rl.size)
    step = n if not chunk_bytes else max(int(chunk_bytes), 1)
    parts = {k: [] for k in ('pcm', 'flags', 'subcode') + (PARITY_ARRAYS if keep else ())}
    tot = dict.fromkeys(COUNTERS, 0)
    at = 0
    while True:
        b = min(at + step, n)
        info = ctx.efmdec_feed(np.asarray(rl[at:b]), final=b >= n)
        for k in COUNTERS:
            tot[k] += info[k]
        for k in parts:
            parts[k].append(ctx.efmdec_read(k, info['samples'] if k in ('pcm', 'flags') else info['frames'])[1])
        if after_feed is not None:
            after_feed()
        at = b
        if at >= n:
            break
    res = {k: np.concatenate(v) for k, v in parts.items()}
    res['counters'] = tot
    return res


def crc16(data):
    """x^16 + x^12 + x^5 + 1, initial value 0, MSB first ("123456789" -> 0x31C3)."""
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x1021) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


def q_decode(sub):
    """Subcode Q of the frames' subcode symbols: a section is 98 frames starting S0, S1; Q is
    bit 6 of the other 96 (MSB first); its last 16 bits are the inverted CRC of the first 80.
    -> sections found, with good CRC, and the first and last mode-1 time code [min, sec, frame]."""
    sub = np.asarray(sub)
    at = np.nonzero((sub[:-1] == SYM_S0) & (sub[1:] == SYM_S1))[0] if sub.size > 1 else ()
    found = good = 0
    times = []
    for a in at:
        if a + 98 > sub.size:
            continue
        found += 1
        by = np.packbits(((sub[a + 2:a + 98] >> 6) & 1).astype(np.uint8))
        if crc16(bytes(by[:10])) ^ 0xFFFF != (int(by[10]) << 8 | int(by[11])):
            continue
        good += 1
        if by[0] & 15 == 1:
            times.append([(int(v) >> 4) * 10 + (int(v) & 15) for v in by[7:10]])
    return {'sections': found, 'crc_good': good, 'first_time': times[0] if times else None,
            'last_time': times[-1] if times else None}


def decode_file(ctx, path, outbase, chunk_bytes=1 << 24, table=None, stats=False, after_feed=None, all_kernels=None):
    """`path`'s run lengths into <outbase>.efm.pcm (s16le stereo, 44.1 kHz) and
    <outbase>.efm.pcm.json; returns the summary.  all_kernels: a dict that receives every kernel's
    time with stats (ldgpu.efmsec reads its own from it)."""
    import json
    import time
    rl = np.memmap(path, dtype=np.uint8, mode='r') if os.path.getsize(path) else np.zeros(0, dtype=np.uint8)
    if stats:
        ctx.profile(True)
    t0 = time.perf_counter()
    res = decode(ctx, rl, chunk_bytes, table, after_feed=after_feed)
    wall = time.perf_counter() - t0
    with open(outbase + '.efm.pcm', 'wb') as fh:
        fh.write(res['pcm'].astype('<i2').tobytes())
    summ = {'run_lengths': int(rl.size), 'sample_rate': 44100}
    summ.update(res['counters'])
    summ['flagged_samples'] = int(res['flags'].any(axis=1).sum()) if res['flags'].size else 0
    summ['q'] = q_decode(res['subcode'])
    if stats:
        summ['wall_s'] = round(wall, 4)
        summ['kernels_ms'] = {k: round(v[1], 3) for k, v in ctx.profile_stats().items() if k.startswith('efmdec_')}
        if all_kernels is not None:
            all_kernels.update({k: round(v[1], 3) for k, v in ctx.profile_stats().items()})
        ctx.profile(False)
    with open(outbase + '.efm.pcm.json', 'w') as fh:
        json.dump(summ, fh, indent=1)
    return summ
