"""FLAC-compressed captures (.ldf, .flac, .oga): the rule of DESIGN.md section 7g restated in plain
Python, bit by bit, plus the encoder and the Ogg muxer that make the test streams.

The bit stream is the public FLAC format (RFC 9639); what is done with a damaged file is this
project's own rule (R0-R6).  The GPU path (csrc/flac_plan.hpp, csrc/flac.hip) is held to
decode() byte for byte: the frame table, the gaps, the counters and the samples."""
import hashlib
import struct

import numpy as np

KEPT, NESTED, MISPLACED = 0, 1, 2
COUNTERS = ('candidates', 'header_ok', 'parsed', 'accepted', 'kept', 'nested', 'misplaced', 'range',
            'ogg_broken', 'lost_bytes', 'gaps', 'gap_samples')
M64 = (1 << 64) - 1


class Refused(Exception):
    """The file is not a stream this project reads (R0)."""


def wrap64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def crc8(data):
    c = 0
    for x in data:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xff if c & 0x80 else (c << 1) & 0xff
    return c


def _crc16_table():
    t = []
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xffff if c & 0x8000 else (c << 1) & 0xffff
        t.append(c)
    return t


CRC16_T = _crc16_table()


def crc16(data):
    c = 0
    for x in data:
        c = ((c << 8) & 0xffff) ^ CRC16_T[(c >> 8) ^ x]
    return c


def coded_number(v):
    """The extended UTF-8 coding of a frame or sample number (1-7 bytes)."""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1):
        n += 1
    assert n <= 7
    out = [((0xff << (8 - n)) & 0xff) | (v >> (6 * (n - 1)))]
    for j in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * j)) & 0x3f))
    return bytes(out)


def parse_streaminfo(b):
    """The 34 bytes of a STREAMINFO block."""
    x = int.from_bytes(b[10:18], 'big')
    return dict(min_bs=int.from_bytes(b[0:2], 'big'), max_bs=int.from_bytes(b[2:4], 'big'),
                min_frame=int.from_bytes(b[4:7], 'big'), max_frame=int.from_bytes(b[7:10], 'big'),
                sample_rate=x >> 44, channels=((x >> 41) & 7) + 1, bps=((x >> 36) & 31) + 1,
                total_samples=x & ((1 << 36) - 1), md5=bytes(b[18:34]).hex())


# ---- R0: the container ----------------------------------------------------------------------------
def ogg_walk(b):
    """The Ogg page walk.  Returns (streaminfo bytes or None, audio packets, ogg_broken, lost) where a
    packet is (file offset of its first byte, its bytes) and lost counts the bytes skipped in
    searching for a page and the pieces of dropped packets."""
    n = len(b)
    pos, serial, last_seq = 0, None, 0
    partial = None                   # the pieces of a packet that continues on the next page
    si, packets, broken, lost = None, [], 0, 0
    first = True

    def emit(pieces):
        nonlocal si, first
        data = b''.join(bytes(b[o:o + l]) for o, l in pieces)
        if not data:
            return
        if first:
            first = False
            if len(data) >= 51 and data[9:13] == b'fLaC' and data[13] & 0x7f == 0 and data[14:17] == b'\0\0\x22':
                si = data[17:51]
            return
        if data[0] != 0xff:
            return                   # a header packet, whatever the stated count
        packets.append((pieces[0][0], data))

    while pos + 27 <= n:
        if b[pos:pos + 4] != b'OggS' or b[pos + 4] != 0:
            q = b.find(b'OggS', pos + 1)
            q = n if q < 0 else q
            lost += q - pos
            pos = q
            continue
        htype, nseg = b[pos + 5], b[pos + 26]
        pserial, seq = struct.unpack_from('<II', b, pos + 14)
        body = pos + 27 + nseg
        blen = sum(b[pos + 27:pos + 27 + nseg]) if body <= n else 0
        if body + blen > n:          # a page cut by the file's end is no page
            lost += n - pos
            pos = n
            break
        lacing = b[pos + 27:body]
        page_end = body + blen
        if serial is None:
            if nseg and blen >= 5 and b[body:body + 5] == b'\x7fFLAC':
                serial = pserial
            else:
                pos = page_end
                continue
        if pserial != serial:
            pos = page_end
            continue
        cont = htype & 1
        k, off = 0, body
        if partial is not None and not (cont and seq == (last_seq + 1) & 0xffffffff):
            broken += 1
            lost += sum(l for _, l in partial)
            partial = None
        if cont and partial is None:
            # the tail of a packet whose head is not here
            while k < nseg:
                lost += lacing[k]
                off += lacing[k]
                k += 1
                if lacing[k - 1] < 255:
                    break
        pieces = partial if partial is not None else []
        partial = None
        start, open_ = off, bool(pieces)
        while k < nseg:
            off += lacing[k]
            open_ = True
            if lacing[k] < 255:
                if off > start:
                    pieces.append((start, off - start))
                emit(pieces)
                pieces, start, open_ = [], off, False
            k += 1
        if open_:
            if off > start:
                pieces.append((start, off - start))
            partial = pieces
        last_seq = seq
        pos = page_end
    else:
        lost += n - pos
    if partial is not None:
        broken += 1
        lost += sum(l for _, l in partial)
    return si, packets, broken, lost


def open_stream(b):
    """R0.  Returns (info, regions, ogg_broken, ogg_lost); a region is (file offset, bytes, single)."""
    b = bytes(b)
    if b[:4] == b'fLaC':
        pos, first = 4, True
        while True:
            if pos + 4 > len(b):
                raise Refused('the metadata is cut short')
            typ, last, ln = b[pos] & 0x7f, b[pos] >> 7, int.from_bytes(b[pos + 1:pos + 4], 'big')
            if first and (typ != 0 or ln != 34):
                raise Refused('the first metadata block is not STREAMINFO')
            if typ == 127:
                raise Refused('metadata block type 127')
            if pos + 4 + ln > len(b):
                raise Refused('the metadata is cut short')
            if first:
                si = b[pos + 4:pos + 38]
            first = False
            pos += 4 + ln
            if last:
                break
        info = parse_streaminfo(si)
        info['container'] = 'native'
        regions, broken, lost = [(pos, b[pos:], False)], 0, 0
    elif b[:4] == b'OggS':
        si, packets, broken, lost = ogg_walk(b)
        if si is None:
            raise Refused('no Ogg FLAC stream with a STREAMINFO block')
        info = parse_streaminfo(si)
        info['container'] = 'ogg'
        regions = [(o, d, True) for o, d in packets]
    elif b[:3] == b'ID3':
        raise Refused('the file begins with an ID3 tag')
    else:
        raise Refused('neither fLaC nor OggS')
    if info['channels'] != 1:
        raise Refused('%d channels' % info['channels'])
    if info['bps'] not in (8, 16):
        raise Refused('%d bits a sample' % info['bps'])
    return info, regions, broken, lost


# ---- R2: the frame header ---------------------------------------------------------------------------
def parse_header(b, c, end, info):
    """The header at b[c:], which may not reach past `end`.  Returns (header bytes, block size,
    number, variable) or None."""
    def need(k):
        return c + k <= end
    if not need(5) or b[c] != 0xff or b[c + 1] not in (0xf8, 0xf9):
        return None
    variable = b[c + 1] & 1
    bsc, src = b[c + 2] >> 4, b[c + 2] & 15
    ch, ssc, res = b[c + 3] >> 4, (b[c + 3] >> 1) & 7, b[c + 3] & 1
    if res or bsc == 0 or src == 15 or ch != 0:
        return None
    if ssc != 0 and ssc != {8: 1, 16: 4}[info['bps']]:
        return None
    x = b[c + 4]
    if x < 0x80:
        nb, v = 1, x
    elif x < 0xc0 or x == 0xff:
        return None
    else:
        nb = 2
        while x & (0x80 >> nb):
            nb += 1
        v = x & (0x7f >> nb)
    if nb > (7 if variable else 6) or not need(4 + nb):
        return None
    for j in range(1, nb):
        y = b[c + 4 + j]
        if y & 0xc0 != 0x80:
            return None
        v = (v << 6) | (y & 0x3f)
    p = c + 4 + nb
    if bsc == 1:
        bs = 192
    elif bsc <= 5:
        bs = 576 << (bsc - 2)
    elif bsc == 6:
        if p + 1 > end:
            return None
        bs = b[p] + 1
        p += 1
    elif bsc == 7:
        if p + 2 > end:
            return None
        bs = ((b[p] << 8) | b[p + 1]) + 1
        p += 2
    else:
        bs = 256 << (bsc - 8)
    p += {12: 1, 13: 2, 14: 2}.get(src, 0)
    if p + 1 > end or bs > info['max_bs']:
        return None
    if crc8(b[c:p]) != b[p]:
        return None
    return p + 1 - c, bs, v, variable


# ---- R3, R4: one frame ----------------------------------------------------------------------------
class Reject(Exception):
    pass


class BitReader:
    def __init__(self, b, bit, limit_bit):
        self.b, self.p, self.lim = b, bit, limit_bit

    def read(self, n):
        if self.p + n > self.lim:
            raise Reject
        if n == 0:
            return 0
        b0, b1 = self.p >> 3, (self.p + n + 7) >> 3
        v = int.from_bytes(self.b[b0:b1], 'big') >> (b1 * 8 - self.p - n)
        self.p += n
        return v & ((1 << n) - 1)

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = 0
        while True:
            if self.p >= self.lim:
                raise Reject
            byte = self.b[self.p >> 3]
            rest = 8 - (self.p & 7)
            x = byte & ((1 << rest) - 1)
            if x:
                z = rest - x.bit_length()
                if self.p + z + 1 > self.lim:
                    raise Reject
                self.p += z + 1
                return q + z
            q += rest
            self.p += rest
            if self.p > self.lim:
                raise Reject


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def decode_frame(b, c, limit, hdr, bs, bps):
    """The subframe, padding and CRC-16 of the frame at c.  Returns (bytes, samples, crc ok);
    raises Reject where R3 rejects."""
    r = BitReader(b, 8 * (c + hdr), 8 * limit)
    if r.read(1):
        raise Reject
    typ = r.read(6)
    wasted = r.unary() + 1 if r.read(1) else 0
    if wasted >= bps:
        raise Reject
    eff = bps - wasted
    if typ == 0:
        s = [r.signed(eff)] * bs
    elif typ == 1:
        s = [r.signed(eff) for _ in range(bs)]
    else:
        if 8 <= typ <= 12:
            order = typ - 8
        elif typ >= 32:
            order = typ - 31
        else:
            raise Reject
        if order > bs:
            raise Reject
        s = [r.signed(eff) for _ in range(order)]
        if typ >= 32:
            prec = r.read(4) + 1
            if prec == 16:
                raise Reject
            shift = r.signed(5)
            if shift < 0:
                raise Reject
            coef = [r.signed(prec) for _ in range(order)]
        else:
            coef, shift = FIXED[order], 0
        method = r.read(2)
        if method > 1:
            raise Reject
        po = r.read(4)
        if not ((po == 0 or bs % (1 << po) == 0) and (bs >> po) >= order):
            raise Reject
        kb, esc = (4, 15) if method == 0 else (5, 31)
        for p in range(1 << po):
            cnt = (bs >> po) - (order if p == 0 else 0)
            k = r.read(kb)
            n = r.read(5) if k == esc else 0
            for _ in range(cnt):
                if k == esc:
                    res = r.signed(n)
                else:
                    u = (r.unary() << k) | r.read(k)
                    res = (u >> 1) ^ -(u & 1)
                i = len(s)
                pred = wrap64(sum(coef[j] * s[i - 1 - j] for j in range(order))) >> shift
                s.append(wrap64(res + pred))
    s = [wrap64(v << wasted) for v in s]
    end = (r.p + 7) >> 3
    if end + 2 > limit:
        raise Reject
    ok = crc16(b[c:end]) == (b[end] << 8 | b[end + 1])
    return end + 2 - c, s, ok


# ---- R1-R6: a file --------------------------------------------------------------------------------
def decode(data, want_samples=True, max_samples=1 << 28):
    """The whole rule.  Returns a dict: info, frames [(offset, bytes, position, block size, state)],
    gaps [(first, count)], counters, n, samples (int16 or uint8 array; None when n > max_samples or
    not wanted)."""
    data = bytes(data)
    info, regions, broken, lost0 = open_stream(data)
    bps = info['bps']
    bypersample = bps // 8
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt['ogg_broken'] = broken
    accepted = []                    # (offset, bytes, position, bs, samples)
    region_bytes = 0
    for roff, b, single in regions:
        region_bytes += len(b)
        cands = [0] if single else [c for c in range(len(b) - 1) if b[c] == 0xff and b[c + 1] in (0xf8, 0xf9)]
        for c in cands:
            cnt['candidates'] += 1
            h = parse_header(b, c, len(b), info)
            if h is None:
                continue
            hdr, bs, num, variable = h
            if not variable and info['min_bs'] != info['max_bs']:
                raise Refused('a fixed-block-size frame in a stream whose STREAMINFO block sizes differ')
            cnt['header_ok'] += 1
            pos = num if variable else num * info['max_bs']
            limit = min(c + 18 + 2 * bs * bypersample, len(b))
            try:
                nbytes, s, ok = decode_frame(b, c, limit, hdr, bs, bps)
            except Reject:
                continue
            if single and c + nbytes != len(b):
                continue
            cnt['parsed'] += 1
            if not ok:
                continue
            if any(v < -(1 << (bps - 1)) or v >= 1 << (bps - 1) for v in s):
                cnt['range'] += 1
                continue
            cnt['accepted'] += 1
            accepted.append((roff + c, nbytes, pos, bs, s))
    frames, placed = [], []
    byte_end, samp_end, kept_bytes = -1, 0, 0
    for off, nbytes, pos, bs, s in accepted:
        if off < byte_end:
            state = NESTED
            cnt['nested'] += 1
        else:
            byte_end = off + nbytes
            if pos < samp_end:
                state = MISPLACED
                cnt['misplaced'] += 1
            else:
                state = KEPT
                cnt['kept'] += 1
                samp_end = pos + bs
                kept_bytes += nbytes
                placed.append((pos, s))
        frames.append((off, nbytes, pos, bs, state))
    n = samp_end
    gaps, at = [], 0
    for pos, s in placed:
        if pos > at:
            gaps.append((at, pos - at))
        at = pos + len(s)
    cnt['gaps'], cnt['gap_samples'] = len(gaps), sum(g[1] for g in gaps)
    cnt['lost_bytes'] = lost0 + region_bytes - kept_bytes
    samples = None
    if want_samples and n <= max_samples:
        samples = np.zeros(n, dtype=np.int64)
        for pos, s in placed:
            samples[pos:pos + len(s)] = s
        samples = samples.astype('<i2') if bps == 16 else (samples + 128).astype(np.uint8)
    return dict(info=info, frames=frames, gaps=gaps, counters=cnt, n=n, samples=samples)


# ---- the encoder ----------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def write(self, v, n):
        if n == 0:
            return
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        if self.n >= 512:
            k = self.n & 7
            self.out += (self.acc >> k).to_bytes((self.n - k) // 8, 'big')
            self.acc &= (1 << k) - 1
            self.n = k

    def unary(self, q):
        while q >= 256:
            self.write(0, 256)
            q -= 256
        self.write(1, q + 1)

    def bytes(self):
        """Zero-padded to a byte."""
        if self.n & 7:
            self.write(0, 8 - (self.n & 7))
        if self.n:
            self.out += self.acc.to_bytes(self.n // 8, 'big')
            self.acc, self.n = 0, 0
        return bytes(self.out)


def rice_k(res):
    """A workable Rice parameter for these residuals."""
    if not len(res):
        return 0
    mean = sum(abs(int(v)) for v in res) / len(res)
    return max(0, int(mean).bit_length())


def encode_subframe(w, s, bps, kind='verbatim', order=0, coef=None, prec=None, shift=0, wasted=0, method=None,
                    po=0, ks=None, escapes=None):
    """One subframe of samples s.  kind: constant, verbatim, fixed or lpc.  ks: a Rice parameter for
    every partition (int or list; None: chosen); escapes: {partition: n} codes those partitions raw
    with n bits.  method None: 0 unless a parameter needs 5 bits."""
    s = [int(v) for v in s]
    bs = len(s)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in s)
        s = [v >> wasted for v in s]
    eff = bps - wasted
    typ = {'constant': 0, 'verbatim': 1, 'fixed': 8 + order, 'lpc': 31 + order}[kind]
    w.write(typ << 1 | (1 if wasted else 0), 8)
    if wasted:
        w.unary(wasted - 1)
    if kind == 'constant':
        assert len(set(s)) == 1
        w.write(s[0], eff)
        return
    if kind == 'verbatim':
        for v in s:
            w.write(v, eff)
        return
    for v in s[:order]:
        w.write(v, eff)
    if kind == 'lpc':
        w.write(prec - 1, 4)
        w.write(shift, 5)
        for cf in coef:
            assert -(1 << (prec - 1)) <= cf < 1 << (prec - 1)
            w.write(cf, prec)
    else:
        coef, shift = FIXED[order], 0
    res = [s[i] - (sum(coef[j] * s[i - 1 - j] for j in range(order)) >> shift) for i in range(order, bs)]
    assert (po == 0 or bs % (1 << po) == 0) and (bs >> po) >= order
    parts, at = [], 0
    for p in range(1 << po):
        cnt = (bs >> po) - (order if p == 0 else 0)
        parts.append(res[at:at + cnt])
        at += cnt
    escapes = escapes or {}
    if ks is None or isinstance(ks, int):
        ks = [rice_k(pt) if ks is None else ks for pt in parts]
    if method is None:
        method = 1 if max(ks) > 14 else 0
    kb, esc = (4, 15) if method == 0 else (5, 31)
    w.write(method, 2)
    w.write(po, 4)
    for p, pt in enumerate(parts):
        if p in escapes:
            n = escapes[p]
            w.write(esc, kb)
            w.write(n, 5)
            for v in pt:
                assert (v == 0) if n == 0 else -(1 << (n - 1)) <= v < 1 << (n - 1)
                w.write(v, n)
            continue
        k = ks[p]
        assert k < esc
        w.write(k, kb)
        for v in pt:
            u = (v << 1) ^ (v >> 63) if v >= 0 else ((-v) << 1) - 1
            w.unary(u >> k)
            w.write(u, k)


BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
            16384: 14, 32768: 15}


def encode_frame(s, bps, number, variable=True, bs_code=None, ss_code=None, check=True, **sub):
    """One frame.  number: the sample number (variable) or the frame number.  bs_code None: the
    short code where the block size has one, else 6 or 7."""
    bs = len(s)
    if bs_code is None:
        bs_code = BS_CODES.get(bs, 6 if bs <= 256 else 7)
    if ss_code is None:
        ss_code = {8: 1, 16: 4}[bps]
    h = bytes([0xff, 0xf9 if variable else 0xf8, bs_code << 4, ss_code << 1]) + coded_number(number)
    if bs_code == 6:
        h += bytes([bs - 1])
    elif bs_code == 7:
        h += struct.pack('>H', bs - 1)
    h += bytes([crc8(h)])
    w = BitWriter()
    encode_subframe(w, s, bps, **sub)
    body = h + w.bytes()
    out = body + struct.pack('>H', crc16(body))
    if check:
        assert len(out) <= 18 + 2 * bs * (bps // 8), 'the frame is longer than the walk bound (R3)'
    return out


def streaminfo(min_bs, max_bs, bps=16, channels=1, total=0, md5=b'\0' * 16, rate=40000):
    x = (rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    return struct.pack('>HH', min_bs, max_bs) + b'\0' * 6 + x.to_bytes(8, 'big') + md5


def meta_block(typ, body, last=False):
    return bytes([typ | (0x80 if last else 0)]) + len(body).to_bytes(3, 'big') + body


def native_stream(si, frames, extra=()):
    """fLaC, STREAMINFO, the extra metadata blocks [(type, body)], the frames."""
    blocks = [(0, si)] + list(extra)
    return b'fLaC' + b''.join(meta_block(t, d, i == len(blocks) - 1) for i, (t, d) in enumerate(blocks)) + \
        b''.join(frames)


def samples_md5(samples, bps=16):
    a = np.asarray(samples)
    return hashlib.md5(a.astype('<i2').tobytes() if bps == 16 else a.astype(np.int8).tobytes()).digest()


# ---- the Ogg muxer --------------------------------------------------------------------------------
def _ogg_crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04c11db7) & 0xffffffff if c & 0x80000000 else (c << 1) & 0xffffffff
        t.append(c)
    return t


OGG_T = _ogg_crc_table()


def ogg_page(serial, seq, lacing, body, cont=False, first=False, last=False, granule=0, crc=True):
    """crc False leaves the page CRC 0 (it is never verified; capture-sized inputs)."""
    h = b'OggS' + bytes([0, (1 if cont else 0) | (2 if first else 0) | (4 if last else 0)]) + \
        struct.pack('<qII', granule, serial, seq) + b'\0\0\0\0' + bytes([len(lacing)]) + bytes(lacing)
    c = 0
    for x in (h + body if crc else b''):
        c = ((c << 8) & 0xffffffff) ^ OGG_T[(c >> 24) ^ x]
    return h[:22] + struct.pack('<I', c) + h[26:] + body


def ogg_pages(packets, serial, payload=4096, flush_each=False, first_seq=0, crc=True):
    """Pages of one logical stream: packets laid into pages of at most `payload` body bytes (whole
    segments, at most 255 a page); flush_each ends the page after every packet."""
    pages, seq = [], first_seq
    lacing, body, cont = [], bytearray(), False

    def flush(next_cont):
        nonlocal lacing, body, cont, seq
        if lacing:
            body = bytes(body)
            pages.append(ogg_page(serial, seq, lacing, body, cont=cont, first=seq == 0, crc=crc))
            seq += 1
        lacing, body, cont = [], bytearray(), next_cont
    for pk in packets:
        segs = [255] * (len(pk) // 255) + [len(pk) % 255]
        at = 0
        for i, sg in enumerate(segs):
            if len(lacing) == 255 or len(body) + sg > max(payload, 255):
                flush(i > 0)
            lacing.append(sg)
            body += pk[at:at + sg]
            at += sg
        if flush_each:
            flush(False)
    flush(False)
    return pages


def ogg_stream(si, frames, serial=0x1d5a, payload=4096, flush_each=False, header_count=1, foreign=None,
               comment=True, crc=True):
    """An Ogg FLAC file: the mapping's first packet alone on the first page, a comment packet, the
    frames one packet each.  foreign: a serial whose pages (of noise) are interleaved."""
    head = b'\x7fFLAC\x01\x00' + struct.pack('>H', header_count) + b'fLaC' + meta_block(0, si, not comment)
    pages = ogg_pages([head], serial)
    rest = ([meta_block(4, b'\0' * 40, True)] if comment else []) + list(frames)
    pages += ogg_pages(rest, serial, payload, flush_each, first_seq=1, crc=crc)
    if foreign is not None:
        rng = np.random.default_rng(7)
        fp = ogg_pages([rng.integers(0, 256, 700, dtype=np.uint8).tobytes() for _ in range(len(pages))], foreign,
                       payload=600)
        out = [fp[0]]
        for i, p in enumerate(pages):
            out.append(p)
            if i + 1 < len(fp):
                out.append(fp[i + 1])
        pages = out
    return b''.join(pages), pages


# ---- the vectorised encoder (capture-sized inputs) --------------------------------------------------
def crc16_rows(rows, lens):
    """CRC-16 of every row's first lens[i] bytes, all rows at once (uint8 [n, m])."""
    t = np.array(CRC16_T, dtype=np.uint16)
    c = np.zeros(rows.shape[0], dtype=np.uint16)
    for j in range(rows.shape[1]):
        nc = (c << 8) ^ t[(c >> 8) ^ rows[:, j]]
        c = np.where(j < lens, nc, c)
    return c


def encode_fast(samples, bs=4096, bps=16, order=2, group=256):
    """A whole capture as a fixed-block-size native stream: fixed prediction of `order` with one Rice
    parameter a frame (order None: verbatim), in numpy.  Returns the file's bytes."""
    si, frames = encode_fast_frames(samples, bs, bps, order, group)
    return b'fLaC' + meta_block(0, si, True) + b''.join(frames)


def encode_fast_frames(samples, bs=4096, bps=16, order=2, group=256):
    """encode_fast's STREAMINFO and frames, for the muxer."""
    a = np.asarray(samples).astype(np.int64)
    if bps == 8:
        a = a - 128
    n = a.size
    nfull = n // bs
    out = []
    coefs = FIXED[order] if order is not None else None
    for g0 in range(0, nfull, group):
        x = a[g0 * bs:min(nfull, g0 + group) * bs].reshape(-1, bs)
        out += _fast_group(x, g0, bs, bps, order, coefs)
    if n % bs:
        out += _fast_group(a[nfull * bs:].reshape(1, -1), nfull, bs, bps, order, coefs)
    md5 = hashlib.md5(a.astype('<i2').tobytes() if bps == 16 else a.astype(np.int8).tobytes()).digest()
    return streaminfo(bs, bs, bps, total=n, md5=md5), out


def _fast_group(x, f0, stream_bs, bps, order, coefs):
    nf, bs = x.shape
    heads = []
    for f in range(nf):
        code = BS_CODES.get(bs, 6 if bs <= 256 else 7)
        h = bytes([0xff, 0xf8, code << 4, {8: 1, 16: 4}[bps] << 1]) + coded_number(f0 + f)
        h += bytes([bs - 1]) if code == 6 else struct.pack('>H', bs - 1) if code == 7 else b''
        heads.append(h + bytes([crc8(h)]))
    hl = np.array([len(h) for h in heads])
    if order is None or bs <= order:
        body = np.zeros((nf, 1 + bs * bps // 8), dtype=np.uint8)
        body[:, 0] = 2
        body[:, 1:] = (x.astype('>i2').view(np.uint8) if bps == 16 else x.astype(np.int8).view(np.uint8)).reshape(nf, -1)
        bl = np.full(nf, body.shape[1])
    else:
        res = x[:, order:].copy()
        for j, cf in enumerate(coefs):
            res -= cf * x[:, order - 1 - j:bs - 1 - j]
        u = np.where(res >= 0, res << 1, ((-res) << 1) - 1)
        k = np.maximum(0, np.ceil(np.log2(np.maximum(u.mean(axis=1), 1))).astype(np.int64) - 1)
        k = np.minimum(k, 30)
        q = u >> k[:, None]
        fixed = 8 + order * bps + 2 + 4 + 5
        nbits = fixed + (q + 1 + k[:, None]).sum(axis=1)
        bl = (nbits + 7) // 8
        bits = np.zeros((nf, int(bl.max()) * 8), dtype=np.uint8)

        def put(col, val, width):
            for j in range(width):
                bits[:, col + j] = (val >> (width - 1 - j)) & 1
        put(0, np.full(nf, (8 + order) << 1), 8)
        for j in range(order):
            put(8 + j * bps, x[:, j] & ((1 << bps) - 1), bps)
        put(8 + order * bps, np.full(nf, 1), 2)           # method 1: 5-bit parameters
        put(10 + order * bps, np.full(nf, 0), 4)
        put(14 + order * bps, k, 5)
        ln = q + 1 + k[:, None]
        start = fixed + np.cumsum(ln, axis=1) - ln
        rows = np.arange(nf)[:, None]
        bits[rows, start + q] = 1
        for j in range(int(k.max())):
            m = k[:, None] > j
            rr, cc = np.nonzero(m & np.ones_like(q, dtype=bool))
            sh = (k[rr] - 1 - j)
            bits[rr, (start + q + 1 + j)[rr, cc]] = (u[rr, cc] >> sh) & 1
        body = np.packbits(bits, axis=1)
    m = int((hl + bl).max())
    rowsb = np.zeros((nf, m), dtype=np.uint8)
    for f in range(nf):
        rowsb[f, :hl[f]] = np.frombuffer(heads[f], dtype=np.uint8)
        rowsb[f, hl[f]:hl[f] + bl[f]] = body[f, :bl[f]]
    crc = crc16_rows(rowsb, hl + bl)
    return [rowsb[f, :hl[f] + bl[f]].tobytes() + struct.pack('>H', int(crc[f])) for f in range(nf)]
