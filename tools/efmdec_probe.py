"""Per-kernel times of the EFM decode on the tests' clean 300-frame
stream tiled to 60 s of disc (441,000 frames), by ldg_profile_*, in calls of 2^22 and 2^24 run
lengths and in one call:

    python tools/efmdec_probe.py [OUT.txt]        (profiles/efmdec_kernels_60s.txt is its output)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ld-decode_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import efmdec_ref as R  # noqa: E402
from ldgpu import efmdec, native  # noqa: E402

rl = R.stream('clean')
_, i1 = R.frame_runs(rl, R.N_FRAMES - 1)
one = rl[:i1]
assert int(one.sum()) == 588 * R.N_FRAMES
tiles = 441000 // R.N_FRAMES
big = np.concatenate([np.tile(one, tiles), rl[i1:]])
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, 'w')


def say(s):
    print(s)
    out.write(s + '\n')
    out.flush()


say('# the clean 300-frame stream tiled %d times: %d frames (60 s of disc), %d run lengths' % (tiles, tiles * R.N_FRAMES, big.size))
ctx = native.Context('NTSC', 0, max_reads=1)
efmdec.decode(ctx, big[:1 << 20])            # warm-up: allocations, code load
for chunk in (1 << 22, 1 << 24, None):
    for rep in range(2):
        ctx.profile(True)
        t0 = time.perf_counter()
        res = efmdec.decode(ctx, big, chunk_bytes=chunk)
        wall = time.perf_counter() - t0
        st = {k: v for k, v in ctx.profile_stats().items() if k.startswith('efmdec_')}
        ctx.profile(False)
        k = res['counters']
        assert k['frames'] == tiles * R.N_FRAMES and k['flagged'] == 0 and k['c2_pass'] == k['frames'] - 109
        tot = sum(v[1] for v in st.values())
        say('chunk %s run %d: wall %.4f s, kernels %.3f ms, %d frames, %d samples' % (chunk, rep, wall, tot, k['frames'], k['samples']))
        for name in sorted(st):
            say('  %-22s launches %5d  %9.3f ms' % (name, st[name][0], st[name][1]))
ctx.close()
out.close()
