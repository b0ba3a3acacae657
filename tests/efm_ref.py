"""EFM run-length extraction (BUILD-DEFINED): the numpy
restatement the GPU (csrc/efm.hip) is held to, and a generator of synthetic EFM under an RF
carrier.  All times are RF samples from sample 0 of the capture file.

    python tests/efm_ref.py --sweep      the loop-gain sweep of DESIGN.md section 7c
"""
import math
import os
import sys

import numpy as np
import scipy.signal as sps
from scipy.special import ndtr

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 'ld-decode_amd')
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from ldgpu.formats import FMT_U8, NAME_TO_FMT, pack_lds, pack_r30, read_samples, samples_in_bytes  # noqa: E402

FS = 40e6
FC = 4321800.0                  # EFM channel clock, Hz
NTAPS = 255
CUTOFF = 1.75e6
DEC = 4
BLOCK = 64                      # decimated samples per baseline block
BASE_HALF = 4                   # blocks either side of the centred mean
L = 1 << 20                     # segment length, RF samples
R = 1 << 16                     # run-in before a segment, RF samples
DELTA = 0.03
ALPHA, BETA = 0.1, 0.002        # the sweep's choice
CANDIDATES = [(1.0, 0.0), (0.5, 0.002), (0.3, 0.005), (0.2, 0.01), (0.1, 0.002), (0.05, 0.001)]
RUN_IN = 1400                   # crossings in R samples (R / (4.8 bits x P0) and some)


def taps(fs=FS):
    return sps.firwin(NTAPS, CUTOFF / (fs / 2))


def samples(raw, fmt):
    """The loader's sample values as float64 (load_sample of csrc/sample.hpp)."""
    buf = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8)
    return read_samples(buf, fmt, 0, samples_in_bytes(fmt, buf.size)).astype(np.float64)


def fir_decimate(x, h):
    """y[m] = sum_k h[k] x[4m + 127 - k], NaN where the window leaves the file."""
    N = x.size
    M = (N // DEC + 1 + BLOCK - 1) // BLOCK * BLOCK
    y = np.full(M, np.nan)
    half = NTAPS // 2
    m_lo = -(-half // DEC)
    m_hi = (N - 1 - half) // DEC if N - 1 - half >= 0 else -1
    if m_hi < m_lo:
        return y
    n = m_hi - m_lo + 1
    acc = np.zeros(n)
    for k in range(NTAPS):
        s0 = DEC * m_lo + half - k
        acc += h[k] * x[s0:s0 + DEC * (n - 1) + 1:DEC]
    y[m_lo:m_hi + 1] = acc
    return y


def baseline(y):
    """z[m] = y[m] - base[m >> 6]; NaN where undefined (a NaN in any of the nine block sums)."""
    B = y.reshape(-1, BLOCK).sum(axis=1)
    nb = B.size
    base = np.full(nb, np.nan)
    w = 2 * BASE_HALF + 1
    if nb >= w:
        s = B[0:nb - w + 1].copy()
        for k in range(1, w):
            s = s + B[k:nb - w + 1 + k]
        base[BASE_HALF:nb - BASE_HALF] = s / (w * BLOCK)
    return y - np.repeat(base, BLOCK)


def crossings(z):
    """(times, m, |z[m-1] - z[m]|) of the sign changes between defined neighbours, in m order."""
    ok = np.isfinite(z)
    neg = z < 0
    m = np.nonzero(ok[1:] & ok[:-1] & (neg[1:] != neg[:-1]))[0] + 1
    a, b = z[m - 1], z[m]
    t = DEC * ((m - 1) + a / (a - b))
    return t, m, np.abs(a - b)


def clock_segment(t, j, alpha, beta, p0, diag=None):
    """Segment j's run over the crossing times t: (bytes, their crossing times, counters)."""
    lo, hi = j * L, (j + 1) * L
    i0 = int(np.searchsorted(t, lo - R, 'left')) if j > 0 else 0
    i1 = int(np.searchsorted(t, hi, 'left'))
    out, when = [], []
    ign = cl = ch = 0
    P = p0
    pmin, pmax = p0 * (1 - DELTA), p0 * (1 + DELTA)
    if i0 < i1:
        ref = float(t[i0])
        for c in t[i0 + 1:i1].tolist():
            d = c - ref
            q = d / P + 0.5
            n = math.floor(q)
            if diag is not None:
                diag[0] = min(diag[0], q - n, n + 1 - q)
            own = c >= lo
            if n < 1:
                ign += own
                continue
            e = d - n * P
            ref = ref + n * P + alpha * e
            P = min(max(P + beta * e / n, pmin), pmax)
            if own:
                cl += n < 3
                ch += n > 11
                out.append(min(max(n, 3), 11))
                when.append(c)
    return (np.array(out, dtype=np.uint8), np.array(when),
            dict(emitted=len(out), ignored=int(ign), clamped_low=int(cl), clamped_high=int(ch), final_P=P))


def n_segments(nsamples):
    return (nsamples + L - 1) // L


def extract(x, seg_lo=0, seg_hi=None, alpha=ALPHA, beta=BETA, fs=FS, h=None):
    """Steps 1-5 over the float64 samples x of a whole file -> dict with bytes, per-segment
    counters, z, the crossing times, and the two conditioning figures."""
    h = taps(fs) if h is None else h
    z = baseline(fir_decimate(x, h))
    t, m, dz = crossings(z)
    seg_hi = n_segments(x.size) if seg_hi is None else seg_hi
    diag = [1.0]
    parts, whens, segs = [], [], []
    for j in range(seg_lo, seg_hi):
        b, w, s = clock_segment(t, j, alpha, beta, fs / FC, diag)
        parts.append(b)
        whens.append(w)
        segs.append(s)
    cat = lambda a, dt: np.concatenate(a) if a else np.zeros(0, dtype=dt)   # noqa: E731
    return dict(bytes=cat(parts, np.uint8), when=cat(whens, np.float64), segments=segs, z=z, times=t,
                min_dz=float(dz.min()) if dz.size else math.inf, min_round=diag[0])


def window(seg_lo, seg_hi, nsamples):
    """[lo, hi) of the file's samples that segments [seg_lo, seg_hi) need (brute force: the
    indices the definition touches, level by level), lo rounded down to a multiple of 12 (the
    packed formats' groups); (0, 0) when nothing is needed."""
    t0, t1 = seg_lo * L - R, seg_hi * L
    # a crossing between m-1 and m lies in [4(m-1), 4m]
    mz = np.arange(max(t0 // DEC - 1, 0), t1 // DEC + 1)
    if mz.size == 0 or nsamples <= 0:
        return 0, 0
    blocks = np.unique(mz >> 6)
    nb = np.unique((blocks[:, None] + np.arange(-BASE_HALF, BASE_HALF + 1)[None, :]).ravel())
    my = (nb[:, None] * BLOCK + np.arange(BLOCK)[None, :]).ravel()
    lo = int(my.min()) * DEC - NTAPS // 2
    hi = int(my.max()) * DEC + NTAPS // 2 + 1
    lo, hi = max(lo, 0), min(hi, nsamples)
    if hi <= lo:
        return 0, 0
    return lo // 12 * 12, hi


# ---- generator ---------------------------------------------------------------------------

def efm_runs(n_frames, rng):
    """Frames of 11, 11 and random run lengths 3..11 filling 588 bits, no 11 beside an 11 in
    the payload or beside the sync."""
    out = []
    for _ in range(n_frames):
        out += [11, 11]
        left = 588 - 22
        prev = 11
        while left:
            hi = 10 if prev == 11 else 11
            ok = [r for r in range(3, hi + 1) if left - r == 0 or left - r >= 3]
            if left <= 11:                      # the last run sits beside the next sync
                ok = [r for r in ok if not (left - r == 0 and r == 11)]
            r = int(rng.choice(ok))
            out.append(r)
            left -= r
            prev = r
    return np.array(out, dtype=np.int64)


def efm_wave(runs, n_samples, t0, clk, fs=FS):
    """(waveform of +-1 smoothed by a Gaussian of sigma 0.45 P0, edge times): edges at
    t0 + bits * P0 / clk."""
    p0 = fs / FC
    edges = t0 + np.concatenate(([0], np.cumsum(runs))) * (p0 / clk)
    edges = edges[edges < n_samples - 64]
    sig = 0.45 * p0
    W = 24
    c = np.ceil(edges).astype(np.int64)
    step = np.zeros(n_samples + 1)
    sign = np.where(np.arange(edges.size) % 2 == 0, -2.0, 2.0)
    np.add.at(step, c, sign)
    w = 1.0 + np.cumsum(step)[:n_samples]
    idx = c[:, None] + np.arange(-W, W)[None, :]
    corr = (ndtr((idx - edges[:, None]) / sig) - (idx >= c[:, None])) * sign[:, None]
    good = (idx >= 0) & (idx < n_samples)
    np.add.at(w, idx[good], corr[good])
    return w, edges


def fm_carrier(n_samples, fs=FS):
    """An 80-LSB 8.1 MHz FM carrier swept +-0.6 MHz at 15.7 kHz plus two 10-LSB tones at the
    NTSC analogue audio carriers."""
    t = np.arange(n_samples) / fs
    fm = 15734.0
    ph = 2 * np.pi * 8.1e6 * t + (0.6e6 / fm) * np.sin(2 * np.pi * fm * t)
    return 80 * np.cos(ph) + 10 * np.cos(2 * np.pi * 2.301e6 * t + 0.3) + 10 * np.cos(2 * np.pi * 2.812e6 * t + 1.1)


MID = {'u8': 128, 's16': 0, 'r30': 512, 'lds': 512}
LIMITS = {'u8': (0, 255), 's16': (-32768, 32767), 'r30': (0, 1023), 'lds': (0, 1023)}


def pack(v, fmt):
    """Rounded sample values -> the format's file bytes."""
    v = np.clip(np.rint(v), *LIMITS[fmt])
    if fmt == 'u8':
        return v.astype(np.uint8).tobytes()
    if fmt == 's16':
        return v.astype('<i2').tobytes()
    return pack_r30(v.astype(np.uint32)) if fmt == 'r30' else pack_lds(v.astype(np.uint16))


def make_efm_capture(n_samples, fmt='u8', clk=1.0, sigma=2.0, amp=12.0, seed=1, carrier=None, t0=300.25):
    """(file bytes, edge times, run lengths): EFM of `amp` LSB under `carrier` (default the FM
    carrier; LSB about the format's mid level), white noise of sigma LSB, rounded."""
    rng = np.random.default_rng(seed)
    p0 = FS / FC
    runs = efm_runs(int(n_samples / (588 * p0 / clk)) + 2, rng)
    w, edges = efm_wave(runs, n_samples, t0, clk)
    car = fm_carrier(n_samples) if carrier is None else carrier
    v = MID[fmt] + car + amp * w + rng.normal(0, sigma, n_samples)
    return pack(v, fmt), edges, runs[:edges.size - 1]


def add_efm(raw_u8, clk=1.0, amp=12.0, seed=1, t0=300.25):
    """EFM added to an existing u8 capture (ldgpu.synth.make_capture's RF as the carrier)."""
    x = np.frombuffer(raw_u8, dtype=np.uint8).astype(np.float64)
    rng = np.random.default_rng(seed)
    runs = efm_runs(int(x.size / (588 * FS / FC / clk)) + 2, rng)
    w, edges = efm_wave(runs, x.size, t0, clk)
    return pack(x + amp * w, 'u8'), edges, runs[:edges.size - 1]


def score(res, edges, runs, skip=RUN_IN):
    """Wrong run lengths past the first `skip` emitted bytes, aligned by time against the true
    edges: an emitted byte whose crossing's nearest edge ends another run length (or lies more
    than half a channel bit away), and a true edge in the scored span no crossing matched.
    Returns (wrong, scored, rms of the matched crossings' distance to their edge)."""
    when, by = res['when'][skip:], res['bytes'][skip:]
    if when.size == 0:
        return 0, 0, 0.0
    k = np.clip(np.searchsorted(edges, when), 1, edges.size - 1)
    k = np.where(np.abs(edges[k - 1] - when) <= np.abs(edges[k] - when), k - 1, k)
    dist = np.abs(edges[k] - when)
    good = (k >= 1) & (dist < 0.5 * FS / FC)
    truth = np.where(k >= 1, runs[np.maximum(k, 1) - 1], 0)
    wrong = int(np.count_nonzero(~good | (truth != by)))
    span = np.arange(k.min(), k.max() + 1)
    wrong += int(span.size - np.unique(k[good]).size)
    return wrong, int(by.size), float(np.sqrt(np.mean(dist[good] ** 2))) if good.any() else 0.0


def sweep(n_runs=20000, out=sys.stdout):
    """Wrong run lengths per candidate (alpha, beta) over clocks 0.985 / 1 / 1.015 and noise
    sigma 2 / 4 / 6 LSB, after the run-in; the choice: fewest wrong in all, ties by fewer wrong
    at sigma 6, then by the smaller rms timing error at sigma 6."""
    h = taps()
    n_samples = int((n_runs + RUN_IN + 600) * 7.1 * FS / FC)
    table = {c: {} for c in CANDIDATES}
    for clk in (0.985, 1.0, 1.015):
        for sigma in (2.0, 4.0, 6.0):
            raw, edges, runs = make_efm_capture(n_samples, 'u8', clk, sigma, seed=int(clk * 1000) + int(sigma))
            z = baseline(fir_decimate(samples(raw, FMT_U8), h))
            t = crossings(z)[0]
            for a, b in CANDIDATES:
                segs = [clock_segment(t, j, a, b, FS / FC) for j in range(n_segments(n_samples))]
                res = dict(bytes=np.concatenate([s[0] for s in segs])[:RUN_IN + n_runs],
                           when=np.concatenate([s[1] for s in segs])[:RUN_IN + n_runs])
                table[a, b][clk, sigma] = score(res, edges, runs)
    keyed = []
    print('alpha beta   | wrong of scored, per (clock, sigma)', file=out)
    for (a, b), row in table.items():
        total = sum(v[0] for v in row.values())
        s6 = sum(v[0] for (c, s), v in row.items() if s == 6.0)
        r6 = max(v[2] for (c, s), v in row.items() if s == 6.0)
        keyed.append((total, s6, r6, a, b))
        print('%-5g %-6g | %s | total %d, sigma 6: %d, rms %.3f' % (
            a, b, ' '.join('%g/%g:%d/%d' % (c, s, v[0], v[1]) for (c, s), v in sorted(row.items())), total, s6, r6),
            file=out)
    best = min(keyed)
    print('chosen: alpha %g beta %g' % (best[3], best[4]), file=out)
    return table, (best[3], best[4])


# ---- the fixtures the CPU and GPU tests share (built once a process) ----------------------

N_FIX = 5 * L // 2 + 1234           # 2.5 segments
FIXTURES = [('u8', 1.0), ('s16', 1.0), ('r30', 1.0), ('lds', 1.0), ('u8', 0.985), ('u8', 1.015)]
SEEDS = {('u8', 1.0): 11, ('s16', 1.0): 12, ('r30', 1.0): 13, ('lds', 1.0): 14, ('u8', 0.985): 15, ('u8', 1.015): 16}
_cache = {}


def fixture(fmt, clk):
    """(file bytes, edges, runs, extract() of the whole file) of the 2.5-segment capture."""
    if (fmt, clk) not in _cache:
        raw, edges, runs = make_efm_capture(N_FIX, fmt, clk, sigma=2.0, seed=SEEDS[fmt, clk])
        _cache[fmt, clk] = (raw, edges, runs, extract(samples(raw, NAME_TO_FMT[fmt])))
    return _cache[fmt, clk]


def spike_fixture():
    """The u8 clock-1 capture with a narrow negative spike in the middle of a positive 11-run
    of segment 1, just deep enough that one decimated sample dips below zero: a pair of
    crossings a fraction of a channel bit apart, which the loop must ignore (n < 1).
    Returns (file bytes, extract())."""
    if 'spike' not in _cache:
        raw, edges, runs, _ = fixture('u8', 1.0)
        x = samples(raw, FMT_U8)
        h = taps()
        k = next(i for i in range(1, runs.size, 2) if runs[i] == 11 and edges[i] > 1.3 * L)
        ms = int(round((edges[k] + edges[k + 1]) / 2 / DEC))
        s0 = (DEC * ms - 256 * 12) // 256 * 256
        ml = ms - s0 // DEC
        xs = x[s0:s0 + 256 * 24]
        c = DEC * ml
        found = None
        for mass in range(1, 1200):
            p = np.full(7, mass // 7, dtype=np.float64)
            p[3 - (mass % 7) // 2:3 - (mass % 7) // 2 + mass % 7] += 1
            t = xs.copy()
            t[c - 3:c + 4] = np.clip(t[c - 3:c + 4] - p, 0, 255)
            z = baseline(fir_decimate(t, h))
            if z[ml] < 0:
                assert z[ml - 1] > 0 and z[ml + 1] > 0, 'the spike is not narrow'
                found = t[c - 3:c + 4]
                break
        assert found is not None
        y = x.copy()
        y[s0 + c - 3:s0 + c + 4] = found
        sraw = pack(y, 'u8')
        _cache['spike'] = (sraw, extract(samples(sraw, FMT_U8)))
    return _cache['spike']


if __name__ == '__main__':
    if '--sweep' in sys.argv:
        sweep()
