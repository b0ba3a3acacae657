"""Kernel times of the EFM run-length extraction (csrc/efm.hip) over an HBM-resident window:
python tools/efm_probe.py [SECONDS=60] [CHUNK_SEGMENTS=64] [OUT.json]

A 0.3 s synthetic NTSC capture (u8) with EFM added (tests/efm_ref.py add_efm) is tiled to
SECONDS in device memory (the joins break the EFM phase every 0.3 s; the work per sample
is what a disc side gives), then ldg_efm_extract runs over it from the device pointer in
calls of CHUNK_SEGMENTS segments with their halo, as ldgpu/efm.py walks a file: once to
warm up, once under ldg_profile_enable.  Prints the per-kernel HIP-event times, the wall
time of the timed pass and the RF Msamples/s of each."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ld-decode_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def main():
    import efm_ref as R
    from ldgpu import efm, native
    from ldgpu.synth import make_capture
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    unit = np.frombuffer(R.add_efm(make_capture(int(40e6 * 0.3), 'u8'), seed=21)[0], dtype=np.uint8)
    reps = max(int(round(seconds * 40e6 / unit.size)), 1)
    n = unit.size * reps
    ctx = native.Context('NTSC', 0, max_reads=1)
    with open('/proc/self/maps') as fh:
        hip = C.CDLL(next(line.split()[-1] for line in fh if 'libamdhip64' in line))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), n) == 0
    for k in range(reps):
        assert hip.hipMemcpy(dev.value + k * unit.size, unit.ctypes.data, unit.size, 1) == 0
    ctx.efm_set_opts(efm.taps())
    nseg = (n + efm.SEG - 1) // efm.SEG

    def one_pass():
        total, segs = 0, []
        for a in range(0, nseg, chunk):
            b = min(a + chunk, nseg)
            lo, hi = native.efm_window(a, b, n)
            by, sg = ctx.efm_extract(None, 0, lo, n, a, b, device_ptr=dev.value + lo, nbytes=n - lo)
            total += by.size
            segs += sg
        return total, segs

    one_pass()
    ctx.profile(True)
    t0 = time.perf_counter()
    total, segs = one_pass()
    wall = time.perf_counter() - t0
    stats = {k: v for k, v in ctx.profile_stats().items() if k.startswith('efm_')}
    ctx.profile(False)
    hip.hipFree(dev)
    ctx.close()
    kern_ms = sum(v[1] for v in stats.values())
    out = {'seconds': n / 40e6, 'samples': n, 'segments': nseg, 'chunk_segments': chunk, 'run_lengths': total,
           'ignored': sum(s['ignored'] for s in segs),
           'kernels': {k: {'launches': v[0], 'total_ms': round(v[1], 3)} for k, v in sorted(stats.items())},
           'kernels_total_ms': round(kern_ms, 3), 'kernels_rf_msamples_per_s': round(n / kern_ms / 1e3, 1),
           'wall_s': round(wall, 4), 'wall_rf_msamples_per_s': round(n / wall / 1e6, 1)}
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 3:
        with open(sys.argv[3], 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
