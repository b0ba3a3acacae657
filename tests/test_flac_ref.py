"""The FLAC rule's Python restatement (tests/flac_ref.py) against the known
answer, the format's anchors, its own encoder, and damage whose effect the test works out itself."""
import hashlib
import math

import numpy as np
import pytest

import flac_cases as K
import flac_ref as F

KNOWN = bytes.fromhex(
    '664c614380000022001000c000000000000009c400f0000000e00acf4e70c513fd712b06dac11800afccfff91008009600fffe5920'
    'fff96008c3800faa02fbb4012cfda80320ff9cfc180190fe0c03840000fc7c01f4fe7003e80064fce08856fff96008c3900ffd1400'
    '0000c6053af9b190886d03a1f0d8647c54cae05987')


def test_known_answer():
    assert len(KNOWN) == 127
    r = F.decode(KNOWN)
    want = [-2] * 192 + [((i * 37) % 23 - 11) * 100 for i in range(16)] + [int(1000 * math.sin(i / 5)) for i in range(16)]
    assert r['samples'].tolist() == want
    assert [(f[2], f[3], f[4]) for f in r['frames']] == [(0, 192, 0), (192, 16, 0), (208, 16, 0)]
    assert r['info']['md5'] == '0acf4e70c513fd712b06dac11800afcc' == hashlib.md5(r['samples'].tobytes()).hexdigest()
    assert r['info']['total_samples'] == 224 == r['n'] and r['info']['sample_rate'] == 40000
    c = r['counters']
    assert (c['candidates'], c['accepted'], c['kept'], c['lost_bytes'], c['gaps']) == (3, 3, 3, 0, 0)


def test_encoder_restates_the_known_answer():
    st = K.Stream()
    st.add([-2] * 192, kind='constant')
    st.add([((i * 37) % 23 - 11) * 100 for i in range(16)], kind='verbatim')
    st.add([int(1000 * math.sin(i / 5)) for i in range(16)], kind='fixed', order=2, method=0, po=1, ks=4)
    assert st.native() == KNOWN


def test_anchors():
    assert F.crc8(b'123456789') == 0xf4 and F.crc16(b'123456789') == 0xfee8
    for v, h in ((127, '7f'), (128, 'c280'), (2047, 'dfbf'), (2048, 'e0a080'), (65536, 'f0908080'),
                 (2 ** 31 - 1, 'fdbfbfbfbfbf'), (2 ** 36 - 1, 'febfbfbfbfbfbf')):
        assert F.coded_number(v).hex() == h
        info = dict(bps=16, max_bs=16, min_bs=16)
        hd = bytes([0xff, 0xf9, 0x60, 0x08]) + F.coded_number(v) + b'\x0f'
        assert F.parse_header(hd + bytes([F.crc8(hd)]), 0, len(hd) + 1, info) == (len(hd) + 1, 16, v, 1)
    hd = bytes([0xff, 0xf8, 0x60, 0x08]) + F.coded_number(2 ** 36 - 1) + b'\x0f'
    assert F.parse_header(hd + bytes([F.crc8(hd)]), 0, len(hd) + 1, info) is None     # 7 bytes: sample numbers only


def clean(r, st, nframes=None):
    c = r['counters']
    n = len(st.frames) if nframes is None else nframes
    assert c['accepted'] == c['kept'] == n and c['nested'] == c['misplaced'] == c['range'] == c['lost_bytes'] == 0
    assert r['gaps'] == K.gaps_of(st.frames)
    assert np.array_equal(r['samples'], st.truth())


@pytest.mark.parametrize('name', ['kinds', 'fixed', 'eight', 'big'])
def test_round_trip(name):
    st = getattr(K, name)()
    r = F.decode(st.native(K.EXTRA))
    clean(r, st)
    assert r['info']['md5'] == hashlib.md5(
        st.truth().tobytes() if st.bps == 16 else (st.truth().astype(np.int16) - 128).astype(np.int8).tobytes()).hexdigest()


def test_numbers():
    a, b, c = K.numbers()
    ra = F.decode(a.native())
    clean(ra, a)
    assert ra['gaps'] == [(0, 126 * 16)] and ra['n'] == 131 * 16
    rb = F.decode(b.native())
    clean(rb, b)
    assert rb['gaps'] == [(0, 2016), (2064, 65504 - 2064)]
    rc = F.decode(c.native())
    assert rc['n'] == (1 << 35) + 16 and rc['samples'] is None and rc['gaps'] == [(16, (1 << 35) - 16)]
    assert rc['counters']['kept'] == 2


def test_adversarial():
    st = K.adversarial()
    r = F.decode(st.native())
    c = r['counters']
    assert c['nested'] == 1 and c['kept'] == 3 and c['candidates'] >= 5 and c['header_ok'] >= 5
    assert np.array_equal(r['samples'], st.truth()) and r['gaps'] == []


@pytest.mark.parametrize('name', ['bitflip', 'removed', 'junk', 'cut', 'zeros', 'metadata_only'])
def test_damage(name):
    data, truth, gaps, kept = K.damaged()[name]
    r = F.decode(data)
    assert r['gaps'] == gaps and r['counters']['kept'] == kept and r['n'] == len(truth)
    assert np.array_equal(r['samples'], truth)
    assert r['counters']['gap_samples'] == sum(g[1] for g in gaps)
    if name == 'junk':
        assert r['counters']['lost_bytes'] == 37
    if name == 'zeros':
        assert r['counters']['lost_bytes'] == 301


def test_ogg():
    for st in (K.kinds(), K.fixed()):
        data, pages = st.ogg(payload=4096)
        assert any(p[5] & 1 for p in pages)                # packets span pages
        r = F.decode(data)
        clean(r, st)
        assert r['counters']['candidates'] == len(st.frames) and r['counters']['ogg_broken'] == 0
    st = K.small_packets()
    for kw in (dict(payload=600), dict(payload=600, foreign=0x77), dict(payload=600, header_count=0),
               dict(payload=255, flush_each=True)):
        clean(F.decode(st.ogg(**kw)[0]), st)
    wide = K.wide_packet()
    data, pages = wide.ogg(payload=255 * 255)
    assert any(p[26] == 255 for p in pages)
    clean(F.decode(data), wide)


def test_ogg_lost_page():
    st = K.small_packets()
    data, pages = st.ogg(payload=255, flush_each=True)
    # pages: the mapping header, the comment, then frame i's page(s); frame 0 (510 bytes) takes two
    lost = 2 + 2 + 2                                       # the page of frame 3
    assert pages[lost][27 + pages[lost][26]:] == st.frames[3][2]
    r = F.decode(b''.join(pages[:lost] + pages[lost + 1:]))
    p, s, _ = st.frames[3]
    assert r['gaps'] == [(p, len(s))] and r['counters']['kept'] == len(st.frames) - 1
    assert np.array_equal(r['samples'], st.truth(skip={3}))
    # the second page of the 510-byte packet lost: that packet is dropped
    r = F.decode(b''.join(pages[:3] + pages[4:]))
    assert r['counters']['ogg_broken'] == 1 and r['gaps'] == [(0, 250)]
    assert np.array_equal(r['samples'], st.truth(skip={0}))


def test_refusals():
    for name, data in K.refusals().items():
        with pytest.raises(F.Refused):
            F.decode(data)
    a, _, _ = K.numbers()
    fr = [f for _, _, f in a.frames]
    with pytest.raises(F.Refused):                         # F8 frames need min == max block size
        F.decode(F.native_stream(F.streaminfo(16, 32), fr))


def test_fast_encoder():
    rng = np.random.default_rng(11)
    s = K.walk(rng, 3 * 4096 + 777).astype('<i2')
    for order in (None, 2):
        data = F.encode_fast(s, bs=4096, order=order)
        r = F.decode(data)
        assert np.array_equal(r['samples'], s) and r['counters']['lost_bytes'] == 0 and r['counters']['kept'] == 4
    u = (K.walk(rng, 1000, amp=100, step=7) + 128).astype(np.uint8)
    assert np.array_equal(F.decode(F.encode_fast(u, bs=256, bps=8, order=1))['samples'], u)
