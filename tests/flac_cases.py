"""The FLAC test streams, built once by the encoder of flac_ref.py and shared by
test_flac_ref.py (CPU) and test_flac_gpu.py.  Every stream comes with the samples it was made from:
`truth` is what the test expects, worked out from what was encoded and what was damaged, never from
a decoder."""
import functools

import numpy as np

import flac_ref as F


def walk(rng, n, amp=6000, step=300):
    """A bounded random walk: a smooth signal whose residuals stay small."""
    s = np.cumsum(rng.integers(-step, step + 1, n))
    return (((s + amp) % (4 * amp)) - 2 * amp).clip(-amp, amp).astype(np.int64)


def lpc_args(rng, order, prec):
    lim = 1 << (prec - 1)
    coef = [int(v) for v in rng.integers(-lim, lim, order)]
    # a shift that keeps the prediction near the signal's own size
    shift = min(15, max(0, prec - 1 + int(np.ceil(np.log2(order)))))
    return dict(kind='lpc', order=order, coef=coef, prec=prec, shift=shift)


class Stream:
    """frames: [(position, samples, encoded bytes)] in file order."""

    def __init__(self, bps=16, variable=True, bs=None):
        self.bps, self.variable, self.bs = bps, variable, bs
        self.frames, self.at = [], 0

    def add(self, s, number=None, **sub):
        s = [int(v) for v in s]
        if self.variable:
            pos = self.at if number is None else number
            num = pos
        else:
            num = self.at // self.bs if number is None else number
            pos = num * self.bs
        self.frames.append((pos, s, F.encode_frame(s, self.bps, num, self.variable, **sub)))
        self.at = pos + len(s)
        return self

    def si(self, md5=True):
        sizes = [len(s) for _, s, _ in self.frames] or [16]
        lo, hi = (self.bs, self.bs) if not self.variable else (min(sizes), max(sizes))
        if self.at > 1 << 28:                      # (a position never read: no total, no MD5)
            return F.streaminfo(lo, hi, self.bps)
        t = self.truth()
        t = t if self.bps == 16 else t.astype(np.int16) - 128       # the MD5 is of the signed samples
        return F.streaminfo(lo, hi, self.bps, total=len(t), md5=F.samples_md5(t, self.bps) if md5 else b'\0' * 16)

    def truth(self, skip=()):
        """The samples of the frames but those numbered in skip, zeros elsewhere."""
        n = max([p + len(s) for i, (p, s, _) in enumerate(self.frames) if i not in skip] or [0])
        out = np.zeros(n, dtype=np.int64)
        for i, (p, s, _) in enumerate(self.frames):
            if i not in skip:
                out[p:p + len(s)] = s
        return out.astype('<i2') if self.bps == 16 else (out + 128).astype(np.uint8)

    def native(self, extra=()):
        return F.native_stream(self.si(), [f for _, _, f in self.frames], extra)

    def ogg(self, **kw):
        return F.ogg_stream(self.si(), [f for _, _, f in self.frames], **kw)


def gaps_of(frames, skip=()):
    """The gaps the kept frames leave: [(first, count)]."""
    out, at = [], 0
    for i, (p, s, _) in enumerate(frames):
        if i in skip:
            continue
        if p > at:
            out.append((at, p - at))
        at = p + len(s)
    return out


@functools.lru_cache(None)
def kinds():
    rng = np.random.default_rng(1)
    st = Stream()
    sizes = [16, 17, 192, 256, 576, 1000, 4096, 4608]
    subs = [dict(kind='constant'), dict(kind='verbatim')] + [dict(kind='fixed', order=o) for o in range(5)]
    for p in range(1, 16):
        subs.append(lpc_args(rng, [1, 2, 8, 12, 32][p % 5], p))
    for i, sub in enumerate(subs):
        bs = sizes[i % len(sizes)]
        if sub.get('order', 0) > bs:
            bs = 192
        s = walk(rng, bs)
        if sub['kind'] == 'constant':
            s = [int(s[0])] * bs
        st.add(s, **sub)
    # Rice methods and parameters
    st.add([7] * 256, kind='fixed', order=1, ks=0, method=0)
    st.add(walk(rng, 576), kind='fixed', order=2, ks=14, method=0)
    st.add(walk(rng, 192), kind='fixed', order=1, ks=15, method=1)
    st.add(walk(rng, 17), kind='fixed', order=0, ks=30, method=1)
    # every partition order of a 256-sample block
    for po in range(9):
        st.add(walk(rng, 256), kind='fixed', order=1, po=po)
    st.add(walk(rng, 4096), kind='lpc', order=8, coef=[3, -2, 1, 0, 1, -1, 0, 1], prec=4, shift=2, po=5)
    # escape partitions: n = 0 (constant), 1 (steps of -1 or 0), 16
    a = walk(rng, 64)
    b = [int(a[-1])] * 64
    c = list(b[-1] + np.cumsum(-rng.integers(0, 2, 64)))
    d = list(rng.integers(-9000, 9000, 64))
    st.add(list(a) + b + c + d, kind='fixed', order=1, po=2, escapes={1: 0, 2: 1, 3: 16})
    # wasted bits
    st.add(walk(rng, 192) * 2, kind='verbatim', wasted=1)
    st.add(walk(rng, 1000, amp=500) * 32, kind='fixed', order=2, wasted=5)
    st.add([64] * 16, kind='constant', wasted=5)
    # full scale
    alt = [32767, -32768] * 96
    st.add(alt, kind='verbatim')
    st.add(alt, kind='fixed', order=0)
    st.add(alt, kind='fixed', order=4)
    # one residual of 3000 at k = 0: a unary run of 6000 zeros
    st.add([0] * 100 + [3000] * 156, kind='fixed', order=1, ks=0, method=0)
    return st


@functools.lru_cache(None)
def fixed():
    rng = np.random.default_rng(2)
    st = Stream(variable=False, bs=4096)
    for _ in range(5):
        st.add(walk(rng, 4096), kind='fixed', order=2)
    st.add(walk(rng, 1234), kind='fixed', order=3)
    return st


@functools.lru_cache(None)
def numbers():
    """(frame numbers 126..130 at 16; sample numbers across 2047/2048 and 65535/65536; one frame at 2^35)"""
    rng = np.random.default_rng(3)
    a = Stream(variable=False, bs=16)
    for k in range(126, 131):
        a.add(walk(rng, 16), number=k, kind='verbatim')
    b = Stream()
    for pos in (2016, 2032, 2048, 65504, 65520, 65536):
        b.add(walk(rng, 16), number=pos, kind='fixed', order=1)
    c = Stream()
    c.add(walk(rng, 16), number=0, kind='verbatim')
    c.add(walk(rng, 16), number=1 << 35, kind='verbatim')
    return a, b, c


@functools.lru_cache(None)
def big():
    rng = np.random.default_rng(4)
    st = Stream()
    st.add(walk(rng, 65535), **lpc_args(rng, 32, 12), po=0)
    return st


@functools.lru_cache(None)
def eight():
    rng = np.random.default_rng(5)
    st = Stream(bps=8)
    st.add(walk(rng, 192, amp=100, step=9), kind='fixed', order=2)
    st.add([-128, 127] * 8, kind='verbatim')
    st.add(walk(rng, 576, amp=120, step=5), **lpc_args(rng, 8, 7))
    st.add([-3] * 17, kind='constant')
    return st


@functools.lru_cache(None)
def adversarial():
    """A verbatim frame whose payload holds (i) a header with a correct CRC-8 followed by noise and
    (ii) a complete valid frame.  Returns (file, truth)."""
    rng = np.random.default_rng(6)
    inner = F.encode_frame([int(v) for v in walk(rng, 16)], 16, 5, kind='verbatim')
    h = bytes([0xff, 0xf9, 0x60, 0x08, 0x07, 0x0f])
    fake = h + bytes([F.crc8(h)]) + rng.integers(0, 255, 41, dtype=np.uint8).tobytes()
    payload = b'\0\1' + fake + b'\0' + inner + b'\0\2'
    payload += b'\0' * (len(payload) % 2)
    st = Stream()
    st.add(walk(rng, 192), kind='fixed', order=2)
    st.add(np.frombuffer(payload, dtype='>i2').astype(np.int64), kind='verbatim')
    st.add(walk(rng, 192), kind='fixed', order=2)
    return st


@functools.lru_cache(None)
def damage_base():
    rng = np.random.default_rng(8)
    st = Stream()
    for i in range(6):
        st.add(walk(rng, 256), kind='fixed', order=2)
    return st


def damaged():
    """name -> (file, truth samples, gaps, kept frames)."""
    st = damage_base()
    fr = [f for _, _, f in st.frames]
    si = st.si()
    out = {}
    flip = bytearray(fr[2])
    flip[len(flip) // 2] ^= 0x10
    out['bitflip'] = (F.native_stream(si, fr[:2] + [bytes(flip)] + fr[3:]), st.truth(skip={2}), [(512, 256)], 5)
    out['removed'] = (F.native_stream(si, fr[:3] + fr[4:]), st.truth(skip={3}), [(768, 256)], 5)
    junk = bytes(range(1, 38))
    out['junk'] = (F.native_stream(si, fr[:2] + [junk] + fr[2:]), st.truth(), [], 6)
    whole = F.native_stream(si, fr)
    out['cut'] = (whole[:len(whole) - len(fr[5]) // 2], st.truth(skip={5}), [], 5)
    out['zeros'] = (F.native_stream(si, [b'\0' * 301] + fr), st.truth(), [], 6)
    out['metadata_only'] = (F.native_stream(si, []), st.truth()[:0], [], 0)
    return out


EXTRA = ((1, b'\0' * 57), (3, b'\0' * 36), (4, b'\x04\0\0\0test\0\0\0\0'))    # padding, seek table, comment


@functools.lru_cache(None)
def small_packets():
    """Frames for the Ogg page cases: one packet of exactly 510 bytes (two full lacing values and a
    closing 0), then 16-sample verbatim frames."""
    rng = np.random.default_rng(9)
    st = Stream()
    st.add(walk(rng, 250), kind='verbatim')        # 7 header bytes + 1 + 500 + 2
    assert len(st.frames[-1][2]) == 510, len(st.frames[-1][2])
    for i in range(10):
        st.add(walk(rng, 16), kind='verbatim')
    return st


@functools.lru_cache(None)
def wide_packet():
    """A packet longer than 255 * 255 bytes: its first page carries 255 segments."""
    rng = np.random.default_rng(10)
    st = Stream()
    st.add(walk(rng, 32768), kind='verbatim')
    st.add(walk(rng, 16), kind='verbatim')
    return st


def refusals():
    st = damage_base()
    fr = [f for _, _, f in st.frames]
    return {
        'stereo': F.native_stream(F.streaminfo(256, 256, 16, channels=2), fr),
        '24bit': F.native_stream(F.streaminfo(256, 256, 24), fr),
        'id3': b'ID3\x04\0\0\0\0\0\x0a' + b'\0' * 10 + st.native(),
        'magic': b'RIFF' + st.native()[4:],
        'no_streaminfo': b'fLaC' + F.meta_block(1, b'\0' * 34, True) + b''.join(fr),
    }
