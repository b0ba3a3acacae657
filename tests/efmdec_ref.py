"""EFM run lengths -> F3 frames -> CIRC -> 44.1 kHz PCM (DESIGN.md section 7d, row F8,
BUILD-DEFINED): the numpy restatement the GPU (csrc/efmdec.hip) is held to byte for byte, and
an independent encoder (PCM -> CIRC -> F3 -> EFM run lengths) that inverts every step.
Everything is integers.  tests/efm_ref.py supplies the RF-level generator."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_PATH = os.path.join(HERE, 'golden', 'efm_map.txt')
S0_BITS, S1_BITS = '00100000000001', '00000000010010'
SYM_S0, SYM_S1, SYM_BAD = 0x100, 0x101, 0xFFFF
FRAME_BITS = 588
MAX_COAST = 7350
LATENCY = 111                       # F3 frames before the first sample


def load_table(path=TABLE_PATH):
    """The 256 code words (14 channel bits, value 0 first) as integers, MSB first."""
    with open(path) as fh:
        words = [ln.strip() for ln in fh if ln.strip()]
    assert len(words) == 256 and all(len(w) == 14 and set(w) <= set('01') for w in words)
    return [int(w, 2) for w in words]


def inverse(table):
    inv = np.full(1 << 14, SYM_BAD, dtype=np.uint16)
    for v, w in enumerate(table):
        inv[w] = v
    inv[int(S0_BITS, 2)] = SYM_S0
    inv[int(S1_BITS, 2)] = SYM_S1
    return inv


# ---- GF(2^8), polynomial 0x11d, alpha = 2 ----------------------------------------------------

EXP = np.zeros(512, dtype=np.int64)
LOG = np.zeros(256, dtype=np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11d
EXP[255:510] = EXP[:255]


def gmul(a, b):
    return 0 if a == 0 or b == 0 else int(EXP[LOG[a] + LOG[b]])


def gdiv(a, b):
    assert b != 0
    return 0 if a == 0 else int(EXP[(LOG[a] - LOG[b]) % 255])


def generator():
    """prod (x - alpha^k), k = 0..3: coefficients, highest power first."""
    g = [1]
    for k in range(4):
        r = int(EXP[k])
        g = [a ^ gmul(b, r) for a, b in zip(g + [0], [0] + g)]
    return g


def syndromes(W):
    """S_k = sum_i W[:, i] alpha^(k (N - 1 - i)), k = 0..3, over the rows of W: [M, 4]."""
    W = np.asarray(W, dtype=np.int64)
    N = W.shape[1]
    e = N - 1 - np.arange(N)
    S = np.zeros((W.shape[0], 4), dtype=np.int64)
    for k in range(4):
        t = np.where(W == 0, 0, EXP[(LOG[W] + k * e[None, :]) % 255])
        S[:, k] = np.bitwise_xor.reduce(t, axis=1)
    return S


def single_error(S, N):
    """(position, value) of the one error the syndromes name, or None."""
    if 0 in S:
        return None
    p = (LOG[S[1]] - LOG[S[0]]) % 255
    if (LOG[S[2]] - LOG[S[1]]) % 255 != p or (LOG[S[3]] - LOG[S[2]]) % 255 != p or p >= N:
        return None
    return N - 1 - int(p), int(S[0])


def crc16(data):
    """x^16 + x^12 + x^5 + 1, initial value 0, MSB first."""
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x1021) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


# ---- decoder -----------------------------------------------------------------------------

def positions(rl):
    return np.concatenate(([0], np.cumsum(np.asarray(rl, dtype=np.int64))))


def frame_grid(rl):
    """Frame starts (channel bits from the first transition) and the sync counters."""
    rl = np.asarray(rl, dtype=np.int64)
    pos = positions(rl)
    ci = np.nonzero((rl[:-1] == 11) & (rl[1:] == 11))[0] if rl.size > 1 else np.zeros(0, dtype=np.int64)
    cand = pos[ci]

    def has(v):
        k = np.minimum(np.searchsorted(cand, v), max(cand.size - 1, 0))
        return cand[k] == v if cand.size else np.zeros(0, dtype=bool)

    conf = cand[has(cand + FRAME_BITS) | has(cand - FRAME_BITS)]
    starts, coasted, breaks = [], 0, 0
    for k in range(conf.size):
        a = int(conf[k])
        if k + 1 == conf.size:
            n = 1
        else:
            n = (2 * (int(conf[k + 1]) - a) + FRAME_BITS) // (2 * FRAME_BITS)
            if n > MAX_COAST:
                n = 1
                breaks += 1
        m = [a + FRAME_BITS * j for j in range(n) if a + FRAME_BITS * j + FRAME_BITS - 4 <= pos[-1]]
        coasted += max(len(m) - 1, 0)
        starts += m
    return np.array(starts, dtype=np.int64), dict(candidates=int(cand.size), confirmed=int(conf.size),
                                                  coasted=coasted, breaks=breaks)


def symbols(rl, starts, inv):
    """(subcode u16[F], F3 bytes u8[F, 32], bad_symbols)."""
    pos = positions(rl)
    F = starts.size
    if F == 0:
        return np.zeros(0, dtype=np.uint16), np.zeros((0, 32), dtype=np.uint8), 0
    bits = np.zeros(int(pos[-1]) + FRAME_BITS + 1, dtype=np.int64)
    bits[pos] = 1
    idx = starts[:, None, None] + 27 + 17 * np.arange(33)[None, :, None] + np.arange(14)[None, None, :]
    val = (bits[idx] << (13 - np.arange(14))[None, None, :]).sum(axis=2)
    sym = inv[val]
    sub = sym[:, 0].copy()
    data = sym[:, 1:]
    bad = data > 255
    return sub, np.where(bad, 0, data).astype(np.uint8), int(bad.sum())


def c1_stage(f3):
    """C1 out u8[F, 28] and erased flag u8[F] (frame 0 has no C1 word: zeros), counters."""
    F = f3.shape[0]
    out = np.zeros((F, 28), dtype=np.uint8)
    flag = np.zeros(F, dtype=np.uint8)
    cnt = dict(c1_pass=0, c1_fixed=0, c1_erased=0)
    if F < 2:
        return out, flag, cnt
    u = f3[1:].astype(np.int64).copy()
    u[:, 0::2] = f3[:-1, 0::2]
    u[:, 12:16] ^= 0xFF
    u[:, 28:32] ^= 0xFF
    S = syndromes(u)
    for i in range(F - 1):
        if not S[i].any():
            cnt['c1_pass'] += 1
            continue
        fix = single_error(S[i], 32)
        if fix is None:
            flag[i + 1] = 1
            cnt['c1_erased'] += 1
        else:
            u[i, fix[0]] ^= fix[1]
            cnt['c1_fixed'] += 1
    out[1:] = u[:, :28]
    return out, flag, cnt


def solve_erasures(S, js, N):
    """Error values Y at positions js from the first len(js) syndromes (Gaussian elimination)."""
    e = len(js)
    X = [int(EXP[N - 1 - j]) for j in js]
    A = [[int(EXP[(LOG[x] * k) % 255]) for x in X] + [int(S[k])] for k in range(e)]
    for c in range(e):
        p = next(r for r in range(c, e) if A[r][c])
        A[c], A[p] = A[p], A[c]
        A[c] = [gdiv(v, A[c][c]) for v in A[c]]
        for r in range(e):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [a ^ gmul(f, b) for a, b in zip(A[r], A[c])]
    return [A[r][e] for r in range(e)]


def c2_word(w, er):
    """One C2 word (28 ints) with erased flags -> (word, flags, outcome)."""
    N = 28
    w = list(w)
    S = syndromes([w])[0]
    js = [j for j in range(N) if er[j]]
    e = len(js)
    if e == 0:
        if not S.any():
            return w, [0] * N, 'c2_pass'
        fix = single_error(S, N)
        if fix is not None:
            w[fix[0]] ^= fix[1]
            return w, [0] * N, 'c2_fixed'
        det = gmul(S[0], S[2]) ^ gmul(S[1], S[1])
        if det:
            s1 = gdiv(gmul(S[0], S[3]) ^ gmul(S[1], S[2]), det)
            s2 = gdiv(gmul(S[1], S[3]) ^ gmul(S[2], S[2]), det)
            roots = [j for j in range(N)
                     if gmul(int(EXP[N - 1 - j]), int(EXP[N - 1 - j])) ^ gmul(s1, int(EXP[N - 1 - j])) ^ s2 == 0]
            if len(roots) == 2:
                x1, x2 = int(EXP[N - 1 - roots[0]]), int(EXP[N - 1 - roots[1]])
                y1 = gdiv(gmul(S[0], x2) ^ int(S[1]), x1 ^ x2)
                t = list(w)
                t[roots[0]] ^= y1
                t[roots[1]] ^= int(S[0]) ^ y1
                if not syndromes([t])[0].any():
                    return t, [0] * N, 'c2_fixed'
        return w, [1] * N, 'c2_failed'
    if e <= 4:
        t = list(w)
        for j, y in zip(js, solve_erasures(S, js, N)):
            t[j] ^= y
        if not syndromes([t])[0].any():
            return t, [0] * N, 'c2_erasure_solved'
        return w, [1] * N, 'c2_failed'
    return w, [int(x) for x in er], 'c2_unsolved'


def c2_stage(c1, c1flag):
    """C2 out u8[F, 28] and per-symbol flags (bit j of u32[F]); words exist for n >= 109."""
    F = c1.shape[0]
    out = np.zeros((F, 28), dtype=np.uint8)
    flags = np.zeros(F, dtype=np.uint32)
    cnt = dict(c2_pass=0, c2_fixed=0, c2_erasure_solved=0, c2_failed=0, c2_unsolved=0)
    if F <= 109:
        return out, flags, cnt
    n = np.arange(109, F)
    src = n[:, None] - 4 * (27 - np.arange(28))[None, :]
    W = c1[src, np.arange(28)[None, :]].astype(np.int64)
    E = c1flag[src]
    S = syndromes(W)
    easy = ~S.any(axis=1) & ~E.any(axis=1)
    for i in range(n.size):
        if easy[i]:
            cnt['c2_pass'] += 1
            out[n[i]] = W[i]
            continue
        w, fl, what = c2_word(W[i], E[i])
        cnt[what] += 1
        out[n[i]] = w
        flags[n[i]] = sum(1 << j for j in range(28) if fl[j])
    return out, flags, cnt


SAMPLE_POS = [0, 16, 2, 18, 4, 20]        # L0 L1 L2 L3 L4 L5 (R: + 6)


def pcm_stage(c2, c2flags):
    """Samples int16[6 (F - 111), 2] and their flags u8 (before concealment)."""
    F = c2.shape[0]
    if F <= LATENCY:
        return np.zeros((0, 2), dtype=np.int16), np.zeros((0, 2), dtype=np.uint8)
    n = np.arange(LATENCY, F)
    pcm = np.zeros((n.size, 6, 2), dtype=np.int16)
    flg = np.zeros((n.size, 6, 2), dtype=np.uint8)
    for t, p0 in enumerate(SAMPLE_POS):
        for ch in range(2):
            p = p0 + 6 * ch
            src = n - 2 if p >= 16 else n
            hi, lo = c2[src, p].astype(np.int64), c2[src, p + 1].astype(np.int64)
            pcm[:, t, ch] = ((hi << 8) | lo).astype(np.uint16).view(np.int16)
            flg[:, t, ch] = ((c2flags[src] >> p) | (c2flags[src] >> (p + 1))) & 1
    return pcm.reshape(-1, 2), flg.reshape(-1, 2)


def conceal(pcm, flags):
    """(samples, counters): a flagged sample between unflagged neighbours -> their mean,
    any other flagged sample -> 0; per channel."""
    out = pcm.copy()
    f = flags.astype(bool)
    n = f.shape[0]
    ok = np.zeros_like(f)
    if n > 2:
        ok[1:-1] = ~f[:-2] & ~f[2:]
    avg = f & ok
    a = np.zeros(pcm.shape, dtype=np.int64)
    if n > 2:
        a[1:-1] = (pcm[:-2].astype(np.int64) + pcm[2:].astype(np.int64)) >> 1
    out[avg] = a[avg].astype(np.int16)
    out[f & ~ok] = 0
    return out, dict(flagged=int(f.sum()), averaged=int(avg.sum()), muted=int((f & ~ok).sum()))


def decode_f3(f3):
    """The CIRC and PCM stages over F3 bytes u8[F, 32]."""
    c1, c1f, k1 = c1_stage(f3)
    c2, c2f, k2 = c2_stage(c1, c1f)
    raw, flags = pcm_stage(c2, c2f)
    pcm, k3 = conceal(raw, flags)
    counters = dict(k1)
    counters.update(k2)
    counters.update(k3)
    return dict(c1=c1, c1_flags=c1f, c2=c2, c2_flags=c2f, pcm=pcm, flags=flags, counters=counters)


def decode(rl, inv=None):
    """The whole rule over run lengths (uint8 array)."""
    inv = inverse(load_table()) if inv is None else inv
    rl = np.asarray(rl, dtype=np.uint8)
    starts, k0 = frame_grid(rl)
    sub, f3, bad = symbols(rl, starts, inv)
    res = decode_f3(f3)
    res['counters'].update(k0)
    res['counters'].update(bad_symbols=bad, frames=int(starts.size), samples=int(res['pcm'].shape[0]))
    res.update(starts=starts, f3=f3, subcode=sub)
    return res


def bcd(v):
    return (v >> 4) * 10 + (v & 15)


def q_decode(sub):
    """Sections (98 frames from S0, S1), their Q CRC, the mode-1 time codes (m, s, f)."""
    sub = np.asarray(sub)
    at = np.nonzero((sub[:-1] == SYM_S0) & (sub[1:] == SYM_S1))[0] if sub.size > 1 else []
    found = good = 0
    times = []
    for a in at:
        if a + 98 > sub.size:
            continue
        found += 1
        q = (sub[a + 2:a + 98] >> 6) & 1
        by = np.packbits(q.astype(np.uint8))
        if crc16(bytes(by[:10])) ^ 0xFFFF != (int(by[10]) << 8 | int(by[11])):
            continue
        good += 1
        if by[0] & 15 == 1:
            times.append((bcd(int(by[7])), bcd(int(by[8])), bcd(int(by[9]))))
    return dict(sections=found, crc_good=good, first_time=times[0] if times else None,
                last_time=times[-1] if times else None)


# ---- encoder (independent of the decoder above: only the field tables are shared) ------------

def _parity_matrix(N, ppos):
    """M [len(data), 4] with parity = xor_i gmul(data[i], M[i]): each data position's unit word
    completed to a code word by solving the four parity checks."""
    rows = []
    H = [[int(EXP[(k * (N - 1 - i)) % 255]) for i in range(N)] for k in range(4)]
    for i in range(N):
        if i in ppos:
            continue
        A = [[H[k][p] for p in ppos] + [H[k][i]] for k in range(4)]      # H_p y = H_i
        for c in range(4):
            r = next(r for r in range(c, 4) if A[r][c])
            A[c], A[r] = A[r], A[c]
            inv = int(EXP[(255 - LOG[A[c][c]]) % 255])
            A[c] = [gmul(v, inv) for v in A[c]]
            for r in range(4):
                if r != c and A[r][c]:
                    f = A[r][c]
                    A[r] = [a ^ gmul(f, b) for a, b in zip(A[r], A[c])]
        rows.append([A[k][4] for k in range(4)])
    return np.array(rows, dtype=np.int64)


def _add_parity(W, N, ppos):
    """Rows of W (data in the non-parity positions) completed to code words."""
    M = _parity_matrix(N, ppos)
    dpos = [i for i in range(N) if i not in ppos]
    D = W[:, dpos]
    for q, p in enumerate(ppos):
        t = np.where(D == 0, 0, EXP[(LOG[D] + LOG[M[:, q]][None, :]) % 255])
        t = np.where(M[None, :, q] == 0, 0, t)
        W[:, p] = np.bitwise_xor.reduce(t, axis=1)
    return W


def q_bytes(section):
    """Mode-1 Q of a section: control 0, ADR 1, track 1, index 1, the running time, CRC."""
    def tobcd(v):
        return (v // 10) << 4 | v % 10
    m, s, f = section // 4500, section // 75 % 60, section % 75
    body = [0x01, 0x01, 0x01, tobcd(m), tobcd(s), tobcd(f), 0, tobcd(m), tobcd(s), tobcd(f)]
    c = crc16(bytes(body)) ^ 0xFFFF
    return body + [c >> 8, c & 255]


def encode_f3(pcm, n_frames):
    """F3 bytes u8[n_frames, 32] whose decode yields `pcm` (int16 [6 (n_frames - 111), 2])."""
    F = n_frames
    nd = max(F - LATENCY, 0)
    assert pcm.shape == (6 * nd, 2)
    by = pcm.astype('>i2').view(np.uint8).reshape(nd, 6, 2, 2)          # frame, t, channel, hi/lo
    D = np.zeros((F + 120, 28), dtype=np.int64)                         # data of PCM frame n at D[n]
    for t, p0 in enumerate(SAMPLE_POS):
        for ch in range(2):
            D[LATENCY:F, p0 + 6 * ch] = by[:, t, ch, 0]
            D[LATENCY:F, p0 + 6 * ch + 1] = by[:, t, ch, 1]
    W2 = np.zeros((F + 112, 28), dtype=np.int64)                        # C2 words 0 .. F + 111
    W2[:, 0:12] = D[:F + 112, 0:12]
    W2[:, 16:28] = D[2:F + 114, 16:28]                                  # (the decoder delays these by two)
    W2 = _add_parity(W2, 28, [12, 13, 14, 15])
    W1 = np.zeros((F + 1, 32), dtype=np.int64)                          # C1 words 0 .. F
    f = np.arange(F + 1)
    for j in range(28):
        W1[:, j] = W2[f + 4 * (27 - j), j]
    W1 = _add_parity(W1, 32, [28, 29, 30, 31])
    W1[:, 12:16] ^= 0xFF
    W1[:, 28:32] ^= 0xFF
    s = np.zeros((F, 32), dtype=np.uint8)
    s[:, 1::2] = W1[:F, 1::2]
    s[:, 0::2] = W1[1:, 0::2]
    return s


def subcode_symbols(n_frames):
    """u16 per frame: S0, S1, then 96 symbols with Q in bit 6."""
    sub = np.zeros(n_frames, dtype=np.uint16)
    for a in range(0, n_frames, 98):
        q = np.unpackbits(np.array(q_bytes(a // 98), dtype=np.uint8))
        blk = np.concatenate(([SYM_S0, SYM_S1], q.astype(np.uint16) << 6))
        sub[a:a + 98] = blk[:n_frames - a]
    return sub


SYNC_BITS = [int(c) for c in '100000000001000000000010']
MERGE = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]


def _merge_ok(prev, merge, nxt, is_sync):
    """The runs across the junction stay in 3..11 and add no 11, 11 pair (a sync's own only)."""
    ones_prev = [i for i, b in enumerate(prev) if b]
    ones_next = [i for i, b in enumerate(nxt) if b]
    take = 3 if is_sync else 2
    win = ones_prev[-2:] + [len(prev) + i for i, b in enumerate(merge) if b] + \
        [len(prev) + 3 + i for i in ones_next[:take]]
    gaps = [b - a for a, b in zip(win[:-1], win[1:])]
    lo = max(len(ones_prev[-2:]) - 1, 0)                 # the gaps from the last one of prev on
    first_next = len(prev) + 3 + ones_next[0]
    cross = [g for a, g in zip(win[lo:-1], gaps[lo:]) if a < first_next]
    if any(g < 3 or g > 11 for g in cross):
        return False
    pairs = sum(1 for a, b in zip(gaps[:-1], gaps[1:]) if a == 11 and b == 11)
    return pairs == (1 if is_sync else 0)


def modulate(f3, sub, table, tail=True):
    """Channel bits -> run lengths (uint8) of the frames, plus a closing sync so the last
    frame is whole."""
    word = {v: [w >> (13 - i) & 1 for i in range(14)] for v, w in enumerate(table)}
    word[SYM_S0] = [int(c) for c in S0_BITS]
    word[SYM_S1] = [int(c) for c in S1_BITS]
    bits = []
    units = []
    for n in range(f3.shape[0]):
        units.append((SYNC_BITS, True))
        units.append((word[int(sub[n])], False))
        units += [(word[int(v)], False) for v in f3[n]]
    if tail:
        units.append((SYNC_BITS, True))
        units.append((word[0], False))
    for k, (u, is_sync) in enumerate(units):
        if k == 0:
            bits += u
            continue
        prev = bits[-40:]
        m = next((m for m in MERGE if _merge_ok(prev, m, u, is_sync)), None)
        assert m is not None, 'no merge bits fit at unit %d' % k
        bits += list(m) + u
    ones = np.nonzero(np.array(bits))[0]
    return np.diff(ones).astype(np.uint8)


def encode(pcm, n_frames, table=None):
    """(run lengths, F3 bytes, subcode symbols) of n_frames frames carrying pcm."""
    table = load_table() if table is None else table
    f3 = encode_f3(pcm, n_frames)
    sub = subcode_symbols(n_frames)
    return modulate(f3, sub, table), f3, sub


# ---- the streams the CPU and GPU tests share (built once a process) --------------------------

N_FRAMES = 300
_cache = {}


def source(n_frames=N_FRAMES, seed=5):
    rng = np.random.default_rng(seed)
    return rng.integers(-32768, 32768, (6 * max(n_frames - LATENCY, 0), 2)).astype(np.int16)


def frame_runs(rl, n):
    """Indices [i0, i1) of the run lengths that lie inside frame n of a clean stream."""
    pos = positions(rl)
    return int(np.searchsorted(pos, FRAME_BITS * n)), int(np.searchsorted(pos, FRAME_BITS * (n + 1)))


def stream(name):
    """Run lengths of the named 300-frame stream: clean, burst24, undetected, slip, lostsync,
    merged."""
    if 'clean' not in _cache:
        pcm = source()
        rl, f3, sub = encode(pcm, N_FRAMES)
        _cache['src'] = (pcm, f3, sub)
        _cache['clean'] = rl
    rl = _cache['clean']
    if name not in _cache:
        pcm, f3, sub = _cache['src']
        if name == 'burst24':
            bad = f3.copy()
            bad[130:154] = np.random.default_rng(24).integers(0, 256, (24, 32))
            out = modulate(bad, sub, load_table())
        elif name == 'undetected':
            # C1 code words added to C1 words: C1 sees nothing, so C2 meets errors without
            # erasures -- one a word (frame 141), two (182, 186), three (223, 227, 231); the
            # three groups differ modulo 4, so they meet in no C2 word
            bad = f3.copy()
            rng = np.random.default_rng(7)
            for n in (141, 182, 186, 223, 227, 231):
                cw = np.zeros((1, 32), dtype=np.int64)
                cw[0, :28] = rng.integers(1, 256, 28)
                cw = _add_parity(cw, 32, [28, 29, 30, 31])[0].astype(np.uint8)
                bad[n - 1, 0::2] ^= cw[0::2]
                bad[n, 1::2] ^= cw[1::2]
            out = modulate(bad, sub, load_table())
        elif name == 'slip':
            out = rl.copy()
            i0, i1 = frame_runs(rl, 150)
            k = next(i for i in range(i0 + 20, i1) if rl[i] < 10)
            out[k] += 1
        elif name == 'lostsync':
            out = rl.copy()
            i0, _ = frame_runs(rl, 160)
            assert rl[i0] == 11 and rl[i0 + 1] == 11
            out[i0], out[i0 + 1] = 10, 12
        elif name == 'merged':
            i0, i1 = frame_runs(rl, 170)
            k = next(i for i in range(i0 + 20, i1 - 3) if rl[i] + rl[i + 1] + rl[i + 2] <= 255)
            out = np.concatenate((rl[:k], [rl[k:k + 3].sum()], rl[k + 3:])).astype(np.uint8)
        else:
            raise KeyError(name)
        _cache[name] = out
    return _cache[name]


def reference(name):
    """decode() of stream(name), computed once."""
    if ('ref', name) not in _cache:
        _cache['ref', name] = decode(stream(name))
    return _cache['ref', name]
