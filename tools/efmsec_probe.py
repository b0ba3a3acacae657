"""Per-kernel times of the EFM decode with the data-sector stage attached (DESIGN.md section
7e) on 60 s of disc: five mode-1 sectors (490 F3 frames) tiled 900 times, 4,500 sectors, clean
and with an 18-frame F3 burst in every tile, by ldg_profile_*, in calls of 2^24 run lengths
and in one call:

    python tools/efmsec_probe.py [OUT.txt]        (profiles/efmsec_kernels_60s.txt is its output)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ld-decode_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import efmdec_ref as R  # noqa: E402
import efmsec_ref as S  # noqa: E402
from ldgpu import efmsec, native  # noqa: E402

PERIOD = 5 * S.SECTOR // 24                  # 490 frames carry five sectors
TILES = 900
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, 'w')


def say(s):
    print(s)
    out.write(s + '\n')
    out.flush()


def runs(f3, closing):
    """The frames' run lengths, up to the next frame's sync (closing: that sync too)."""
    rl = R.modulate(f3, R.subcode_symbols(f3.shape[0]), R.load_table())
    if closing:
        return rl
    i1 = int(np.searchsorted(R.positions(rl), 588 * f3.shape[0]))
    assert int(rl[:i1].sum()) == 588 * f3.shape[0]
    return rl[:i1]


def stream(burst):
    """A lead-in of 111 frames and one period, then the steady-state period tiled: the CIRC
    encoder reaches 111 frames, so its output repeats with the bytes from frame 111 on."""
    F = R.LATENCY + 3 * PERIOD
    by = np.resize(S.plain_sectors()[1].reshape(-1), 24 * (F - R.LATENCY))
    f3 = R.encode_f3(S.to_pcm(by), F)
    head, tile = f3[:R.LATENCY + PERIOD], f3[R.LATENCY + PERIOD:R.LATENCY + 2 * PERIOD].copy()
    assert np.array_equal(tile, f3[R.LATENCY:R.LATENCY + PERIOD])
    if burst:
        tile[150:150 + burst] = np.random.default_rng(burst).integers(0, 256, (burst, 32))
    return np.concatenate([runs(head, False), np.tile(runs(tile, False), TILES - 2), runs(tile, True)])


ctx = native.Context('NTSC', 0, max_reads=1)
for burst in (0, 18):
    big = stream(burst)
    say('# five sectors tiled %d times, an F3 burst of %d frames a tile: %d run lengths' % (TILES, burst, big.size))
    efmsec.decode(ctx, big[:1 << 20])            # warm-up: allocations, code load
    for chunk in (1 << 24, None):
        for rep in range(2):
            ctx.profile(True)
            t0 = time.perf_counter()
            pcm, res = efmsec.decode(ctx, big, chunk_bytes=chunk)
            wall = time.perf_counter() - t0
            st = {k: v for k, v in ctx.profile_stats().items() if k.startswith(('efmdec_', 'efmsec_'))}
            ctx.profile(False)
            k = res['counters']
            assert k['sectors'] == 5 * TILES and k['bad'] == 0 and k['other'] == 0, k
            assert (k['corrected'] > TILES) if burst else (k['good'] == 5 * TILES and k['coasted'] == 0), k
            dec = sum(v[1] for n, v in st.items() if n.startswith('efmdec_'))
            sec = sum(v[1] for n, v in st.items() if n.startswith('efmsec_'))
            say('chunk %s run %d: wall %.4f s, efmdec kernels %.3f ms, efmsec kernels %.3f ms, %s' % (chunk, rep, wall, dec, sec, k))
            for name in sorted(st):
                if name.startswith('efmsec_'):
                    say('  %-22s launches %5d  %9.3f ms' % (name, st[name][0], st[name][1]))
ctx.close()
out.close()
