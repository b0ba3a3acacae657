"""Kernel time of the disc stacker (ldg_k_stack) by the library's own
event timing: N in {2, 4, 8, 16} sources, 16 NTSC frames a call, after a warm-up call.
Achieved bytes/s = (N + 1) x 955,500 x 16 over the kernel time.

    python tools/stack_probe.py [OUT.json] [--calls K]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ld-decode_amd'))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12      # MI355X HBM3E: the spec peak, a float4 copy as measured
FRAMES = 16


def main():
    from ldgpu import native
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    calls = int(sys.argv[sys.argv.index('--calls') + 1]) if '--calls' in sys.argv else 5
    W, H = 910, 525
    rng = np.random.default_rng(1)
    base = rng.integers(0, 65536, (FRAMES, H * W)).astype(np.int32)
    rows = []
    ctx = native.Context('NTSC', 0, max_reads=1, max_frames=FRAMES)
    try:
        for n in (2, 4, 8, 16):
            srcs = [np.clip(base + rng.integers(-4000, 4001, base.shape), 0, 65535).astype(np.uint16) for _ in range(n)]
            # a dropout a field or so per source, as a clean disc has them; and none at all
            runs = np.zeros((FRAMES, n, 2, native.MAX_LINES, 8, 2), dtype=np.int16)
            counts = np.zeros((FRAMES, n, 2, native.MAX_LINES), dtype=np.int32)
            for f in range(FRAMES):
                for s in range(n):
                    p, r = int(rng.integers(0, 2)), int(rng.integers(22, 260))
                    runs[f, s, p, r, 0] = (300, 420)
                    counts[f, s, p, r] = 1
            for label, rc in (('few runs', (runs, counts)), ('no run arrays', (None, None))):
                for mode in ('smart-mean', 'median', 'mean'):
                    ctx.stack_frames(srcs, None, *rc, mode=mode)                 # warm-up
                    ctx.profile(True)
                    for _ in range(calls):
                        ctx.stack_frames(srcs, None, *rc, mode=mode)
                    launches, ms = ctx.profile_stats()['stack']
                    ctx.profile(False)
                    t = ms / launches / 1e3
                    nbytes = (n + 1) * W * H * 2 * FRAMES
                    rows.append({'n_src': n, 'mode': mode, 'runs': label, 'launches': launches, 'kernel_us': round(t * 1e6, 2),
                                 'bytes': nbytes, 'GB_per_s': round(nbytes / t / 1e9, 1),
                                 'share_of_8.0_TBps_spec': round(nbytes / t / HBM_SPEC, 3),
                                 'share_of_6.29_TBps_copy': round(nbytes / t / HBM_COPY, 3)})
                    print(json.dumps(rows[-1]), flush=True)
    finally:
        ctx.close()
    out = {'what': 'ldg_k_stack kernel time by ldg_profile_enable (HIP events around each launch), %d NTSC frames a call, '
                   'mean of %d calls after a warm-up call' % (FRAMES, calls),
           'library_source_sha256': native.lib_source_hash(), 'rows': rows}
    if args:
        with open(args[0], 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
