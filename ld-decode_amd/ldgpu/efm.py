"""EFM (digital audio) run lengths from the RF on the GPU (csrc/efm.hip; BUILD-DEFINED,
DESIGN.md section 7c): walk a capture file in chunks of whole segments, each with the halo it
needs, concatenate the bytes, and summarise them.

The output is one byte per run length (3..11 channel bits): what this project understands
later ld-decode versions to write as <outfile>.efm, the input of the EFM decode (F3 frames,
CIRC, PCM: ldgpu/efmdec.py).
"""
import numpy as np

from . import native
from .formats import samples_in_bytes

SEG = native.EFM_SEG
CUTOFF_HZ = 1.75e6


def taps(fs=40e6):
    """The low-pass: firwin(255, 1.75 MHz), built on the host like rfparams.py's tables."""
    import scipy.signal as sps
    return sps.firwin(native.EFM_NTAPS, CUTOFF_HZ / (fs / 2))


def segment_range(start_sample, end_sample, nsamples):
    """A requested sample range [start, end) widened outward to whole segments and cut to the
    file: (seg_lo, seg_hi)."""
    nseg = (nsamples + SEG - 1) // SEG
    lo = max(int(start_sample), 0) // SEG
    hi = nseg if end_sample is None else min((max(int(end_sample), 0) + SEG - 1) // SEG, nseg)
    return min(lo, hi), hi


def sample_byte(fmt, s):
    """Byte offset of sample s (on a packing group: a multiple of 12 always is)."""
    return {0: s, 1: 2 * s, 2: s // 3 * 4, 3: s // 4 * 5}[fmt]


def extract(ctx, raw, fmt, seg_lo=0, seg_hi=None, chunk_segments=64, fs=40e6, opts=None):
    """The bytes of segments [seg_lo, seg_hi) of the capture `raw` (uint8 array of the whole
    file, e.g. a np.memmap) and the per-segment counters.  ctx: a native.Context."""
    nsamples = samples_in_bytes(fmt, raw.size)
    if seg_hi is None:
        seg_hi = (nsamples + SEG - 1) // SEG
    ctx.efm_set_opts(taps(fs), fs=fs, **(opts or {}))
    parts, segs = [], []
    step = max(int(chunk_segments), 1)
    for a in range(seg_lo, seg_hi, step):
        b = min(a + step, seg_hi)
        lo, hi = native.efm_window(a, b, nsamples)
        b0 = sample_byte(fmt, lo)
        b1 = raw.size if hi >= nsamples else sample_byte(fmt, (hi + 11) // 12 * 12)
        by, sg = ctx.efm_extract(np.asarray(raw[b0:b1]), fmt, lo, nsamples, a, b)
        parts.append(by)
        segs += sg
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), segs


def summarise(T, segs, seg_lo=0, fs=40e6):
    """The .efm.json record: counts, the 3..11 histogram, the segments' final period over the
    nominal one, and the frame check that needs no code table -- syncs (positions i with
    T[i] == T[i + 1] == 11) and frames_588 (consecutive syncs 588 channel bits apart)."""
    T = np.asarray(T, dtype=np.uint8)
    p0 = fs / native.EFM_CHANNEL_HZ
    hist = np.bincount(T, minlength=12)
    syncs = np.nonzero((T[:-1] == 11) & (T[1:] == 11))[0] if T.size > 1 else np.zeros(0, dtype=np.int64)
    frames = 0
    if syncs.size > 1:
        cs = np.concatenate(([0], np.cumsum(T, dtype=np.int64)))
        frames = int(np.count_nonzero(cs[syncs[1:]] - cs[syncs[:-1]] == 588))
    rel = [s['final_P'] / p0 for s in segs]
    return {'first_segment': int(seg_lo), 'segments': len(segs), 'segment_samples': SEG,
            'run_lengths': int(T.size), 'histogram': {str(k): int(hist[k]) for k in range(3, 12)},
            'ignored': int(sum(s['ignored'] for s in segs)),
            'clamped_low': int(sum(s['clamped_low'] for s in segs)),
            'clamped_high': int(sum(s['clamped_high'] for s in segs)),
            'final_period_ratio': ({'min': min(rel), 'mean': float(np.mean(rel)), 'max': max(rel)} if rel else None),
            'syncs': int(syncs.size), 'frames_588': frames}


def extract_file(ctx, path, outbase, start_sample=0, end_sample=None, chunk_segments=64, fmt=None, stats=False):
    """`path`'s run lengths for the sample range into <outbase>.efm and <outbase>.efm.json;
    returns the summary."""
    import json
    import time
    from .formats import fmt_from_path
    fmt = fmt_from_path(path) if fmt is None else fmt
    raw = np.memmap(path, dtype=np.uint8, mode='r')
    nsamples = samples_in_bytes(fmt, raw.size)
    a, b = segment_range(start_sample, end_sample, nsamples)
    if stats:
        ctx.profile(True)
    t0 = time.perf_counter()
    T, segs = extract(ctx, raw, fmt, a, b, chunk_segments)
    wall = time.perf_counter() - t0
    with open(outbase + '.efm', 'wb') as fh:
        fh.write(T.tobytes())
    summ = summarise(T, segs, a)
    summ['samples'] = [a * SEG, min(b * SEG, nsamples)]
    if stats:
        summ['wall_s'] = round(wall, 4)
        summ['kernels_ms'] = {k: round(v[1], 3) for k, v in ctx.profile_stats().items() if k.startswith('efm_')}
        ctx.profile(False)
    with open(outbase + '.efm.json', 'w') as fh:
        json.dump(summ, fh, indent=1)
    return summ
