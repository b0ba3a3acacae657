"""EFM data sectors (BUILD-DEFINED): the numpy / plain Python
restatement the GPU (csrc/efmsec.hip) is held to byte for byte -- the byte stream before
concealment with per-byte erasures, the 2352-byte sector grid, descrambling, the EDC and the
Reed-Solomon product code of CD-ROM mode 1 (ECMA-130) -- and an independent encoder (sector ->
EDC -> RSPC parity from the check equations -> scramble -> bytes as s16le -> efmdec_ref.encode).
Everything is integers.  tests/efmdec_ref.py supplies the field tables and the CIRC layers."""
import numpy as np

import efmdec_ref as R
from efmdec_ref import EXP, LOG, gdiv, gmul

SECTOR = 2352
MAX_COAST = 75
MAX_ROUNDS = 8
SYNC = bytes([0] + [255] * 10 + [0])
GOOD, CORRECTED, BAD, OTHER = 0, 1, 2, 3
COUNTERS = ('sectors', 'candidates', 'confirmed', 'coasted', 'breaks', 'good', 'corrected', 'bad', 'other', 'p_fixed',
            'q_fixed', 'erased_bytes')
REC = np.dtype([('status', '<i4'), ('rounds', '<i4'), ('erased', '<i4'), ('minute', 'u1'), ('second', 'u1'),
                ('frame', 'u1'), ('mode', 'u1')])


# ---- step 1: the bytes -------------------------------------------------------------------

def bytes_of(c2, c2flags):
    """(bytes u8[24 (F - 111)], erased u8): frame n >= 111 in the order of the .efm.pcm file
    before concealment, a byte erased if its own C2 flag bit is set."""
    F = c2.shape[0]
    if F <= R.LATENCY:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)
    n = np.arange(R.LATENCY, F)
    by = np.zeros((n.size, 6, 2, 2), dtype=np.uint8)                     # frame, t, channel, low / high
    er = np.zeros((n.size, 6, 2, 2), dtype=np.uint8)
    for t, p0 in enumerate(R.SAMPLE_POS):
        for ch in range(2):
            p = p0 + 6 * ch
            src = n - 2 if p >= 16 else n
            by[:, t, ch, 1], by[:, t, ch, 0] = c2[src, p], c2[src, p + 1]
            er[:, t, ch, 1], er[:, t, ch, 0] = (c2flags[src] >> p) & 1, (c2flags[src] >> (p + 1)) & 1
    return by.reshape(-1), er.reshape(-1)


# ---- step 4: the scrambler ---------------------------------------------------------------

def scramble_seq():
    """The 2340 bytes of the register x^15 + x + 1, preset 0x0001, LSB first."""
    reg, out = 1, []
    for _ in range(SECTOR - 12):
        b = 0
        for k in range(8):
            b |= (reg & 1) << k
            reg = (reg >> 1) | (((reg ^ (reg >> 1)) & 1) << 14)
        out.append(b)
    return np.array(out, dtype=np.uint8)


SCR = scramble_seq()


# ---- step 5: the EDC ---------------------------------------------------------------------

EDC_POLY = 0xD8018001
_T = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ EDC_POLY if _c & 1 else _c >> 1
    _T.append(_c)


def edc(data):
    c = 0
    for b in bytes(data):
        c = _T[(c ^ b) & 255] ^ (c >> 8)
    return c


def verified(sec):
    """Mode byte 1 and the EDC of bytes 0..2063 equal to bytes 2064..2067 (little-endian)."""
    return int(sec[15]) == 1 and edc(sec[:2064]) == int.from_bytes(bytes(sec[2064:2068]), 'little')


# ---- step 6: the product code --------------------------------------------------------------

def _p_index():
    s = 43 * np.arange(26)[None, :] + np.arange(43)[:, None]            # [word n, i]
    return np.stack([12 + 2 * s + h for h in range(2)])                 # [h, n, i]


def _q_index():
    n = np.arange(26)[:, None]
    s = np.concatenate(((44 * np.arange(43)[None, :] + 43 * n) % 1118, 1118 + n, 1144 + n), axis=1)
    return np.stack([12 + 2 * s + h for h in range(2)])


P_IDX = _p_index().reshape(86, 26)          # byte index of symbol i of word (h, n): row 43 h + n
Q_IDX = _q_index().reshape(52, 45)          # row 26 h + n


def word_syndromes(W):
    """S0 = sum c[i], S1 = sum c[i] alpha^(N - 1 - i) over the rows of W."""
    W = np.asarray(W, dtype=np.int64)
    e = W.shape[1] - 1 - np.arange(W.shape[1])
    t = np.where(W == 0, 0, EXP[(LOG[W] + e[None, :]) % 255])
    return np.bitwise_xor.reduce(W, axis=1), np.bitwise_xor.reduce(t, axis=1)


def fix_word(c, f, N):
    """One word in place (c: values, f: erasure flags, lists of N) -> changed."""
    S0 = S1 = 0
    for i in range(N):
        S0 ^= c[i]
        S1 ^= gmul(c[i], int(EXP[N - 1 - i]))
    js = [i for i in range(N) if f[i]]
    if len(js) == 0:
        if S0 == 0 or S1 == 0:
            return False
        p = int((LOG[S1] - LOG[S0]) % 255)
        if p >= N:
            return False
        c[N - 1 - p] ^= S0
        return True
    if len(js) == 1:
        j = js[0]
        if gmul(S0, int(EXP[N - 1 - j])) != S1:
            return False
        c[j] ^= S0
        f[j] = 0
        return True
    if len(js) == 2:
        x1, x2 = int(EXP[N - 1 - js[0]]), int(EXP[N - 1 - js[1]])
        y1 = gdiv(gmul(S0, x2) ^ S1, x1 ^ x2)
        c[js[0]] ^= y1
        c[js[1]] ^= S0 ^ y1
        f[js[0]] = f[js[1]] = 0
        return True
    return False


def rspc_pass(sec, fl, IDX):
    """One pass over the words IDX (in place) -> words fixed."""
    W = sec[IDX].astype(np.int64)
    F = fl[IDX]
    S0, S1 = word_syndromes(W)
    fixed = 0
    for r in np.nonzero((S0 != 0) | (S1 != 0) | F.any(axis=1))[0]:
        c, f = [int(v) for v in W[r]], [int(v) for v in F[r]]
        if fix_word(c, f, IDX.shape[1]):
            sec[IDX[r]] = c
            fl[IDX[r]] = f
            fixed += 1
    return fixed


# ---- step 2: the grid ----------------------------------------------------------------------

def sector_grid(by):
    """Sector starts and the grid's counters over the whole stream."""
    by = np.asarray(by, dtype=np.uint8)
    n = by.size
    if n >= 12:
        ok = np.ones(n - 11, dtype=bool)
        for k, v in enumerate(SYNC):
            ok &= by[k:n - 11 + k] == v
        cand = np.nonzero(ok)[0].astype(np.int64)
    else:
        cand = np.zeros(0, dtype=np.int64)
    s = set(cand.tolist())
    conf = [c for c in cand.tolist() if c + SECTOR in s or c - SECTOR in s]
    starts, coasted, breaks = [], 0, 0
    for k, a in enumerate(conf):
        if k + 1 == len(conf):
            m = 1
        else:
            m = (2 * (conf[k + 1] - a) + SECTOR) // (2 * SECTOR)
            if m > MAX_COAST:
                m = 1
                breaks += 1
        got = [a + SECTOR * j for j in range(m) if a + SECTOR * j + SECTOR <= n]
        coasted += max(len(got) - 1, 0)
        starts += got
    return np.array(starts, dtype=np.int64), dict(candidates=int(cand.size), confirmed=len(conf), coasted=coasted,
                                                  breaks=breaks)


# ---- steps 3 to 8 --------------------------------------------------------------------------

def fix_sector(raw, er):
    """One sector's 2352 bytes and erasure flags -> (sector out, record fields, p_fixed, q_fixed)."""
    sec = np.array(raw, dtype=np.uint8)
    fl = np.array(er, dtype=np.uint8)
    sec[:12] = np.frombuffer(SYNC, dtype=np.uint8)
    fl[:12] = 0
    sec[12:] ^= SCR
    erased = int(fl[12:].sum())
    plain = sec.copy()
    status, rounds, pf, qf = BAD, 0, 0, 0
    if not fl[12:2068].any() and verified(sec):
        status = GOOD
    else:
        while rounds < MAX_ROUNDS:
            rounds += 1
            a = rspc_pass(sec, fl, P_IDX)
            b = rspc_pass(sec, fl, Q_IDX)
            pf += a
            qf += b
            if verified(sec):
                status = CORRECTED
                break
            if a + b == 0:
                break
        if status != CORRECTED:
            sec = plain
            status = OTHER if int(plain[15]) != 1 and not er[12:16].any() else BAD
    return sec, (status, rounds, erased, int(sec[12]), int(sec[13]), int(sec[14]), int(sec[15])), pf, qf


def feed(by, er):
    """The whole stage over a byte stream and its erasure flags."""
    by = np.asarray(by, dtype=np.uint8)
    er = (np.asarray(er) != 0).astype(np.uint8)
    starts, k = sector_grid(by)
    ns = starts.size
    sectors = np.zeros((ns, SECTOR), dtype=np.uint8)
    rec = np.zeros(ns, dtype=REC)
    k.update(sectors=ns, good=0, corrected=0, bad=0, other=0, p_fixed=0, q_fixed=0, erased_bytes=0)
    for i, a in enumerate(starts):
        sectors[i], r, pf, qf = fix_sector(by[a:a + SECTOR], er[a:a + SECTOR])
        rec[i] = r
        k[('good', 'corrected', 'bad', 'other')[r[0]]] += 1
        k['p_fixed'] += pf
        k['q_fixed'] += qf
        k['erased_bytes'] += r[2]
    return dict(starts=starts, records=rec, sectors=sectors, data=sectors[:, 16:2064].copy(), counters=k)


def decode_f3(f3):
    """F3 bytes -> the sector stage's result, with the byte stream ('bytes', 'erased')."""
    res = R.decode_f3(f3)
    by, er = bytes_of(res['c2'], res['c2_flags'])
    out = feed(by, er)
    out.update(bytes=by, erased=er)
    return out


def decode(rl):
    """Run lengths -> the sector stage's result."""
    return decode_f3(R.decode(rl)['f3'])


# ---- encoder (independent of the decoder: only the field tables are shared) ----------------

def tobcd(v):
    return (v // 10) << 4 | v % 10


def _parity2(c, N):
    """The last two symbols of a word from sum c[i] = 0 and sum c[i] alpha^(N - 1 - i) = 0."""
    A = B = 0
    for i in range(N - 2):
        A ^= c[i]
        B ^= gmul(c[i], int(EXP[N - 1 - i]))
    y1 = gdiv(A ^ B, 3)                       # y1 (alpha + 1) = A + B,  y1 + y2 = A
    return y1, A ^ y1


def encode_sector(user, address, mode=1):
    """The 2352 scrambled bytes of a sector: header (BCD minute, second, frame of `address`,
    mode), 2048 user bytes, EDC, 8 zeros, P and Q parity."""
    sec = np.zeros(SECTOR, dtype=np.uint8)
    sec[:12] = np.frombuffer(SYNC, dtype=np.uint8)
    sec[12:16] = [tobcd(address // 4500), tobcd(address // 75 % 60), tobcd(address % 75), mode]
    sec[16:2064] = user
    sec[2064:2068] = np.frombuffer(edc(sec[:2064]).to_bytes(4, 'little'), dtype=np.uint8)
    for h in range(2):
        pl = [int(v) for v in sec[12 + h::2]]                            # plane symbols 0..1169
        for n in range(43):
            idx = [43 * m + n for m in range(26)]
            pl[idx[24]], pl[idx[25]] = _parity2([pl[s] for s in idx], 26)
        for n in range(26):
            idx = [(44 * m + 43 * n) % 1118 for m in range(43)] + [1118 + n, 1144 + n]
            pl[idx[43]], pl[idx[44]] = _parity2([pl[s] for s in idx], 45)
        sec[12 + h::2] = pl
    sec[12:] ^= scramble_seq()
    return sec


def to_pcm(by):
    """A byte stream (a multiple of 24 long) as the samples whose s16le file it is."""
    return np.frombuffer(np.asarray(by, dtype=np.uint8).tobytes(), dtype='<i2').reshape(-1, 2).copy()


# ---- the streams the CPU and GPU tests share (built once a process) --------------------------

N_SECTORS = 5
OFFSET = 40
N_FRAMES = 605
_cache = {}


def plain_sectors(n=N_SECTORS, seed=11, mode=1):
    """n sectors' (user bytes u8[n, 2048], scrambled bytes u8[n, 2352]), addresses from 00:02:00."""
    rng = np.random.default_rng(seed)
    user = rng.integers(0, 256, (n, 2048)).astype(np.uint8)
    return user, np.stack([encode_sector(user[i], 150 + i, mode) for i in range(n)])


def stream_bytes():
    """(bytes u8[24 (605 - 111)], user): the five sectors from byte 40, seeded noise around them."""
    if 'bytes' not in _cache:
        user, sec = plain_sectors()
        by = np.random.default_rng(12).integers(0, 256, 24 * (N_FRAMES - R.LATENCY)).astype(np.uint8)
        by[OFFSET:OFFSET + sec.size] = sec.reshape(-1)
        _cache['bytes'] = (by, user)
    return _cache['bytes']


def stream_f3(burst=0, start=150):
    """The 605 F3 frames of the shared stream, `burst` frames from `start` replaced by noise."""
    if 'f3' not in _cache:
        _cache['f3'] = R.encode_f3(to_pcm(stream_bytes()[0]), N_FRAMES)
    f3 = _cache['f3'].copy()
    if burst:
        f3[start:start + burst] = np.random.default_rng(1000 * start + burst).integers(0, 256, (burst, 32))
    return f3


def burst_result(burst, start=150):
    """decode_f3 of the shared stream with an F3 burst, computed once."""
    key = ('res', burst, start)
    if key not in _cache:
        _cache[key] = decode_f3(stream_f3(burst, start))
    return _cache[key]


def exact(res):
    """Every sector the stage passed as good or corrected carries the source's data."""
    user = stream_bytes()[1]
    idx = (res['starts'] - OFFSET) // SECTOR
    return all(np.array_equal(res['data'][i], user[idx[i]])
               for i in range(idx.size) if res['records']['status'][i] in (GOOD, CORRECTED))


def all_sound(res):
    return res['starts'].size == N_SECTORS and bool(np.all(res['records']['status'] <= CORRECTED)) and exact(res)


def first_failing(start=150, upto=40):
    """The smallest burst at `start` after which a sector is neither good nor corrected."""
    key = ('fail', start)
    if key not in _cache:
        _cache[key] = next((b for b in range(1, upto + 1) if not all_sound(burst_result(b, start))), None)
    return _cache[key]


def stream_rl(burst=0, start=150):
    """Run lengths of the shared stream (through the EFM modulator)."""
    key = ('rl', burst, start)
    if key not in _cache:
        _cache[key] = R.modulate(stream_f3(burst, start), R.subcode_symbols(N_FRAMES), R.load_table())
    return _cache[key]


def stage_case(name):
    """(bytes, erased, user data) of the named stage-level case: three sectors from byte 100
    (five for 'header'), the middle one damaged, unless said otherwise."""
    if ('case', name) in _cache:
        return _cache['case', name]
    ns = 5 if name == 'header' else 3
    user, sec = plain_sectors(ns, seed=21)
    by = np.random.default_rng(22).integers(0, 256, 100 + ns * SECTOR + 77).astype(np.uint8)
    by[100:100 + ns * SECTOR] = sec.reshape(-1)
    er = np.zeros(by.size, dtype=np.uint8)
    a = 100 + SECTOR * (ns // 2)                                         # the middle sector
    rng = np.random.default_rng(23)
    if name.startswith('erased'):                                        # erased172, erased200, erased258
        n = int(name[6:])
        by[a + 500:a + 500 + n] = rng.integers(0, 256, n)
        er[a + 500:a + 500 + n] = 1
    elif name.startswith('errors'):                                      # errors<seed>: 8 unflagged errors
        at = np.random.default_rng(int(name[6:])).choice(np.arange(12, SECTOR), 8, replace=False)
        by[a + at] ^= np.random.default_rng(int(name[6:]) + 100).integers(1, 256, 8).astype(np.uint8)
    elif name == 'header':                                               # a wrong, flagged sync between two good ones
        by[a:a + 12] = rng.integers(0, 256, 12)
        er[a:a + 12] = 1
    elif name == 'planted':                                              # the pattern inside scrambled data
        by[a + 1000:a + 1012] = np.frombuffer(SYNC, dtype=np.uint8)
    elif name == 'mode2':
        by[a:a + SECTOR] = plain_sectors(3, seed=21, mode=2)[1][1]
    elif name == 'empty':
        by, er = by[:0], er[:0]
    elif name == 'nosync':
        by = rng.integers(1, 255, 6000).astype(np.uint8)
        er = np.zeros(by.size, dtype=np.uint8)
    else:
        raise KeyError(name)
    _cache['case', name] = (by, er, user)
    return _cache['case', name]


STAGE_CASES = ['erased172', 'erased200', 'erased258'] + ['errors%d' % s for s in range(10)] + \
    ['header', 'planted', 'mode2', 'empty', 'nosync']


def stage_result(name):
    if ('caseres', name) not in _cache:
        by, er, _ = stage_case(name)
        _cache['caseres', name] = feed(by, er)
    return _cache['caseres', name]
