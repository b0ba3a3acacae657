"""The restatement of the EFM data-sector rule (tests/efmsec_ref.py, DESIGN.md section 7e, row
F9) against its own, independent encoder: the known answers of the scrambler and the EDC, the
product code's check equations, the shared 605-frame stream clean and under F3 bursts, and the
stage-level cases the GPU test repeats.  CPU only."""
import numpy as np
import pytest

import efmdec_ref as R
import efmsec_ref as S

STARTS = (150, 151, 152, 153, 200, 230)


def test_scrambler_known_answers():
    seq = S.scramble_seq()
    assert seq.size == 2340
    assert bytes(seq[:16]) == bytes.fromhex('018000600028001E80086006A802FE81')
    assert bytes(seq[-4:]) == bytes.fromhex('72DDE599')


def test_edc_known_answer_and_polynomial():
    assert S.edc(b'123456789') == 0x6EC2EDC4
    # (x^16 + x^15 + x^2 + 1)(x^16 + x^2 + x + 1) over GF(2), and its reflection without x^32
    a, b, prod = 0x18005, 0x10007, 0
    for k in range(17):
        if b >> k & 1:
            prod ^= a << k
    assert prod == 0x18001801B
    assert int(format(prod & 0xFFFFFFFF, '032b')[::-1], 2) == S.EDC_POLY == 0xD8018001


def test_every_word_of_an_encoded_sector_checks():
    user, sec = S.plain_sectors(2, seed=3)
    for i, s in enumerate(sec):
        d = s.copy()
        assert bytes(d[:12]) == S.SYNC
        d[12:] ^= S.SCR
        assert S.verified(d) and np.array_equal(d[16:2064], user[i])
        for idx in (S.P_IDX, S.Q_IDX):
            S0, S1 = S.word_syndromes(d[idx])
            assert not S0.any() and not S1.any()
    # the P words tile bytes 12..2247, the Q words bytes 12..2351, each once
    assert sorted(S.P_IDX.reshape(-1)) == list(range(12, 2248))
    assert sorted(S.Q_IDX.reshape(-1)) == list(range(12, 2352))


def test_bytes_are_the_pcm_file_before_concealment():
    res = R.decode_f3(S.stream_f3())
    by, er = S.bytes_of(res['c2'], res['c2_flags'])
    assert by.tobytes() == res['pcm'].astype('<i2').tobytes() == S.stream_bytes()[0].tobytes() and not er.any()
    # per byte: a flag on one byte of a sample erases that byte alone
    fl = res['c2_flags'].copy()
    fl[300] |= 1 << 1                                     # C2 position 1: the low byte of L0 of frame 300
    _, er = S.bytes_of(res['c2'], fl)
    assert er.sum() == 1 and er[24 * (300 - R.LATENCY)] == 1


def test_clean_stream():
    res = S.burst_result(0)
    assert np.array_equal(res['starts'], S.OFFSET + S.SECTOR * np.arange(5))
    assert np.all(res['records']['status'] == S.GOOD) and np.array_equal(res['data'], S.stream_bytes()[1])
    assert [tuple(r)[3:] for r in res['records']] == [(0, 2, f, 1) for f in range(5)]
    k = res['counters']
    assert (k['sectors'], k['candidates'], k['confirmed'], k['good'], k['coasted']) == (5, 5, 5, 5, 0)
    # through the modulator and back
    got = S.decode(S.stream_rl())
    assert np.array_equal(got['sectors'], res['sectors']) and got['counters'] == k


@pytest.mark.parametrize('start', STARTS)
def test_f3_bursts(start):
    """Bursts of up to 15 F3 frames never reach the sector stage (section 7d's threshold); from
    16 on the product code repairs what CIRC flagged; whatever passes as good or corrected is
    the source's data at every burst length.  The smallest failing burst is recorded in DESIGN.md
    section 7e: 22, 21, 22, 22, 18, 21 frames for these starts."""
    fail = None
    for b in range(1, 41):
        res = S.burst_result(b, start)
        assert S.exact(res), (start, b)
        if b <= 15:
            assert res['starts'].size == 5 and np.all(res['records']['status'] == S.GOOD), (start, b)
        if fail is None and not S.all_sound(res):
            fail = b
    print('start %d: first failing burst %s' % (start, fail))
    assert fail is None or fail >= 17
    assert fail == S.first_failing(start)


def middle(res):
    i = res['starts'].size // 2
    return res['records'][i], res['data'][i], res['sectors'][i]


@pytest.mark.parametrize('n, rounds', [(172, 1), (200, None)])
def test_erased_runs_are_repaired(n, rounds):
    res = S.stage_result('erased%d' % n)
    rec, data, _ = middle(res)
    user = S.stage_case('erased%d' % n)[2]
    assert rec['status'] == S.CORRECTED and np.array_equal(res['data'], user) and rec['erased'] == n
    assert rec['rounds'] == 1 if rounds else rec['rounds'] > 1


def test_an_erased_run_too_long_is_passed_on_unchanged():
    by, er, _ = S.stage_case('erased258')
    res = S.stage_result('erased258')
    rec, _, sec = middle(res)
    assert rec['status'] == S.BAD and res['counters']['bad'] == 1
    plain = by[100 + S.SECTOR:100 + 2 * S.SECTOR].copy()
    plain[12:] ^= S.SCR
    assert np.array_equal(sec, plain)


@pytest.mark.parametrize('seed', range(10))
def test_unflagged_errors_are_repaired(seed):
    res = S.stage_result('errors%d' % seed)
    assert middle(res)[0]['status'] == S.CORRECTED and np.array_equal(res['data'], S.stage_case('errors%d' % seed)[2])


def test_a_damaged_header_is_coasted_over():
    res = S.stage_result('header')
    k = res['counters']
    assert (k['sectors'], k['candidates'], k['confirmed'], k['coasted'], k['good']) == (5, 4, 4, 1, 5)
    assert np.array_equal(res['data'], S.stage_case('header')[2])
    assert bytes(res['sectors'][2][:12]) == S.SYNC


def test_a_planted_pattern_is_never_confirmed():
    res = S.stage_result('planted')
    k = res['counters']
    assert (k['candidates'], k['confirmed'], k['sectors']) == (4, 3, 3)
    assert np.array_equal(res['data'], S.stage_case('planted')[2])       # and the product code removes it


def test_mode_2_is_passed_on_as_other():
    by, _, _ = S.stage_case('mode2')
    rec, _, sec = middle(S.stage_result('mode2'))
    plain = by[100 + S.SECTOR:100 + 2 * S.SECTOR].copy()
    plain[12:] ^= S.SCR
    assert rec['status'] == S.OTHER and rec['mode'] == 2 and np.array_equal(sec, plain)


@pytest.mark.parametrize('name', ['empty', 'nosync'])
def test_inputs_without_sectors(name):
    res = S.stage_result(name)
    assert res['starts'].size == 0 and res['data'].shape == (0, 2048) and not any(res['counters'].values())
