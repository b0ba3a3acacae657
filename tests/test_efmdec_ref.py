"""The EFM decode's definition on the CPU: the code table, the field
and CRC known answers, and the numpy restatement (tests/efmdec_ref.py) against its independent
encoder -- clean streams, burst errors up to the threshold DESIGN.md states, random errors,
damaged run lengths, short streams, concealment."""
import numpy as np
import pytest

import efmdec_ref as R
from ldgpu import efmdec

BURST_STARTS = (130, 131, 132, 133, 150)


@pytest.fixture(scope='module')
def clean():
    rl = R.stream('clean')
    pcm, f3, sub = R._cache['src']
    return rl, pcm, f3, sub


def test_table():
    t = R.load_table()
    assert len(set(t)) == 256 and format(t[0], '014b') == '01001000100000'
    for w in t:
        b = format(w, '014b')
        assert '11' not in b and '101' not in b and '0' * 11 not in b and '1' in b
    s0, s1 = int(R.S0_BITS, 2), int(R.S1_BITS, 2)
    assert s0 not in t and s1 not in t and s0 != s1
    inv = R.inverse(t)
    assert [int(inv[w]) for w in t] == list(range(256))
    assert inv[s0] == R.SYM_S0 and inv[s1] == R.SYM_S1
    assert np.count_nonzero(inv != R.SYM_BAD) == 258
    # the product's loader and inverse are the same table
    assert efmdec.load_table() == t and np.array_equal(efmdec.inverse_table(t), inv)


def test_known_answers():
    g = R.generator()
    assert g == [1, 15, 54, 120, 64]
    assert [int(R.LOG[c]) for c in g] == [0, 75, 249, 78, 6]
    assert R.crc16(b'123456789') == 0x31C3 == efmdec.crc16(b'123456789')
    # a code word has zero syndromes, for both lengths and parity places
    for n, pp in ((28, [12, 13, 14, 15]), (32, [28, 29, 30, 31])):
        w = np.random.default_rng(n).integers(0, 256, (5, n))
        w[:, pp] = 0
        assert not R.syndromes(R._add_parity(w.astype(np.int64), n, pp)).any()


def test_clean_stream_round_trips(clean):
    rl, pcm, f3, sub = clean
    assert rl.min() >= 3 and rl.max() <= 11
    res = R.reference('clean')
    k = res['counters']
    assert k['frames'] == R.N_FRAMES and k['samples'] == 6 * (R.N_FRAMES - 111) == pcm.shape[0]
    assert k['candidates'] == k['confirmed'] == R.N_FRAMES + 1 and k['coasted'] == 0 and k['breaks'] == 0
    assert np.array_equal(res['starts'], 588 * np.arange(R.N_FRAMES))
    assert np.array_equal(res['f3'], f3) and np.array_equal(res['subcode'], sub) and k['bad_symbols'] == 0
    assert np.array_equal(res['pcm'], pcm) and not res['flags'].any()
    assert k['c1_pass'] == R.N_FRAMES - 1 and k['c2_pass'] == R.N_FRAMES - 109
    q = R.q_decode(res['subcode'])
    assert q == dict(sections=3, crc_good=3, first_time=(0, 0, 0), last_time=(0, 0, 2))
    pq = efmdec.q_decode(res['subcode'])
    assert (pq['sections'], pq['crc_good'], pq['first_time'], pq['last_time']) == (3, 3, [0, 0, 0], [0, 0, 2])


def burst(f3, s, b):
    bad = f3.copy()
    bad[s:s + b] = np.random.default_rng(1000 * s + b).integers(0, 256, (b, 32))
    return R.decode_f3(bad)


@pytest.mark.parametrize('s', BURST_STARTS)
def test_bursts_12_and_24(clean, s):
    _, pcm, f3, _ = clean
    r = burst(f3, s, 12)
    assert np.array_equal(r['pcm'], pcm) and not r['flags'].any()
    r = burst(f3, s, 24)
    wrong = r['pcm'] != pcm
    assert r['flags'].any() and not (wrong & (r['flags'] == 0)).any()


def test_burst_threshold(clean):
    """Over B = 1 .. 30 frames of random bytes at the five starts: no unflagged wrong sample
    anywhere, and one threshold T with every burst up to T exact and unflagged and every longer
    one flagged.  DESIGN.md section 7d states T = 15."""
    _, pcm, f3, _ = clean
    exact = {}
    for b in range(1, 31):
        for s in BURST_STARTS:
            r = burst(f3, s, b)
            wrong = r['pcm'] != pcm
            assert not (wrong & (r['flags'] == 0)).any(), (s, b)
            exact[s, b] = not wrong.any() and not r['flags'].any()
    last_exact = max(b for b in range(1, 31) if all(exact[s, b] for s in BURST_STARTS))
    first_flagged = min(b for b in range(1, 31) if not any(exact[s, b] for s in BURST_STARTS))
    print('last exact burst %d frames, first flagged at every start %d' % (last_exact, first_flagged))
    assert all(exact[s, b] for s in BURST_STARTS for b in range(1, last_exact + 1))
    assert 12 <= last_exact < 24 and first_flagged == last_exact + 1
    assert last_exact == 15


def test_random_single_symbol_errors(clean):
    _, pcm, f3, _ = clean
    rng = np.random.default_rng(60)
    bad = f3.copy()
    for _ in range(60):
        bad[rng.integers(0, R.N_FRAMES), rng.integers(0, 32)] ^= rng.integers(1, 256)
    r = R.decode_f3(bad)
    assert np.array_equal(r['pcm'], pcm) and not r['flags'].any()
    assert r['counters']['c1_fixed'] + r['counters']['c1_erased'] > 50


def test_errors_c1_cannot_see(clean):
    """Code words added to C1 words reach C2 as errors without erasures: one and two a word are
    corrected, three are not (the word fails or, rarely, is miscorrected: a distance-5 code)."""
    _, pcm, _, _ = clean
    r = R.reference('undetected')
    k = r['counters']
    assert k['c1_pass'] == R.N_FRAMES - 1 and k['c2_erasure_solved'] == k['c2_unsolved'] == 0
    # 28 words with one error; 27 with two and 2 with one; those with three that the 300 frames hold
    assert k['c2_fixed'] >= 28 + 29 and k['c2_failed'] > 0 and k['flagged'] > 0
    wrong = (r['pcm'] != pcm).any(axis=1)
    first_triple = 6 * (223 - 111)                     # samples before the first word with three errors
    assert not wrong[:first_triple].any() and not r['flags'][:first_triple].any()


@pytest.mark.parametrize('name', ['slip', 'lostsync', 'merged'])
def test_run_length_damage(clean, name):
    rl, pcm, _, _ = clean
    bad = R.stream(name)
    assert bad.size != rl.size or (bad != rl).any()
    r = R.reference(name)
    assert r['counters']['frames'] == R.N_FRAMES
    assert np.array_equal(r['pcm'], pcm) and not r['flags'].any()
    if name == 'lostsync':
        assert r['counters']['coasted'] == 1 and r['counters']['confirmed'] == R.N_FRAMES
    if name == 'slip':
        assert r['counters']['c1_erased'] >= 1


@pytest.mark.parametrize('frames,samples', [(111, 0), (112, 6)])
def test_short_streams(frames, samples):
    pcm = R.source(frames, seed=frames)
    rl, _, _ = R.encode(pcm, frames)
    r = R.decode(rl)
    assert r['counters']['frames'] == frames and r['pcm'].shape == (samples, 2)
    assert np.array_equal(r['pcm'], pcm) and not r['flags'].any()


def test_empty_and_syncless_streams():
    r = R.decode(np.zeros(0, dtype=np.uint8))
    assert r['counters']['frames'] == 0 and r['pcm'].shape == (0, 2) and r['subcode'].size == 0
    rl = np.random.default_rng(3).integers(3, 11, 5000).astype(np.uint8)       # no 11 at all
    r = R.decode(rl)
    assert r['counters']['candidates'] == 0 and r['counters']['frames'] == 0 and r['pcm'].shape == (0, 2)
    rl[100:102] = 11                                                           # a candidate nothing confirms
    r = R.decode(rl)
    assert r['counters']['candidates'] == 1 and r['counters']['confirmed'] == 0 and r['counters']['frames'] == 0


def test_concealment():
    pcm = np.array([[100, -100], [7, 7], [201, -301], [5, 5], [9, 9], [1000, 2000], [-32768, 32767]], dtype=np.int16)
    flags = np.array([[0, 0], [1, 1], [0, 0], [1, 0], [1, 0], [0, 0], [1, 1]], dtype=np.uint8)
    out, k = R.conceal(pcm, flags)
    # between unflagged neighbours: the mean, shifted arithmetically ((-100 - 301) >> 1 = -201)
    assert out[1].tolist() == [150, -201]
    # beside another flagged sample, or at the stream's end: muted
    assert out[3].tolist() == [0, 5] and out[4].tolist() == [0, 9] and out[6].tolist() == [0, 0]
    assert out[[0, 2, 5]].tolist() == pcm[[0, 2, 5]].tolist()
    assert k == dict(flagged=6, averaged=2, muted=4)
    first, _ = R.conceal(pcm[:1], np.ones((1, 2), dtype=np.uint8))
    assert first.tolist() == [[0, 0]]
