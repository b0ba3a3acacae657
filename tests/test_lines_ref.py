"""The NTSC line services' rule (tests/lines_ref.py) on the CPU: known
answers on ideal rows at the edges of every comparison in the rule, and the table of captures
through the oracle's whole RF chain: what the table says each read decodes to, and the robustness
condition that lets the GPU (held to +-1 LSB of the oracle's .tbc) be held to the same record."""
import numpy as np
import pytest

import lines_ref as R
from lines_ref import ABSENT, CHECK, FRAME, OK, T25, T35, T50


# ---- the start search ---------------------------------------------------------------------------
@pytest.mark.parametrize('xs,found', [(269, False), (270, True), (409, True), (410, False)])
def test_caption_start_window(xs, found):
    # all-ones bytes: no later rise that 40 quiet pixels precede
    rec = R.captions(R.ideal_cc(xs, 0xFF, 0xFF))
    if found:
        assert (rec['cc_x'], rec['cc']) == (xs, (0xFF, 0xFF)) and rec['cc_state'] == CHECK
    else:
        assert rec == dict(cc_state=ABSENT, cc_runin=0, cc_x=-1, cc=(0, 0))


@pytest.mark.parametrize('xr,found', [(59, False), (60, True), (159, True), (160, False)])
def test_video_id_start_window(xr, found):
    word = R.vid_word(0x3FFF)
    rec = R.video_id(R.ideal_vid(xr, word))
    if found:
        assert rec == dict(vid_state=OK, vid_x=xr, vid_bits=word)
    elif xr < 60:
        # the next rise 20 quiet pixels precede is cell 2's, where the cells read 1, 1
        assert rec['vid_x'] == xr + 64 and rec['vid_state'] == FRAME
    else:
        assert rec == dict(vid_state=ABSENT, vid_x=-1, vid_bits=0)


def test_quiet_run_of_exactly_q():
    p = R.ideal_cc(339, 0xFF, 0xFF, rises=6)
    q = p.copy()
    q[339 - 41] = T25 + 1                        # p[299 .. 338]: 40 quiet pixels
    rec = R.captions(q)
    assert rec['cc_x'] == 339 and rec['cc_runin'] == 7
    q = p.copy()
    q[339 - 40] = T25 + 1                        # 39
    assert R.captions(q)['cc_state'] == ABSENT
    word = R.vid_word(0)
    p = R.ideal_vid(100, word)
    q = p.copy()
    q[40:100 - 20] = T35 + 1                     # a plateau from before the window (no rise in it): 20 quiet
    assert R.video_id(q) == dict(vid_state=OK, vid_x=100, vid_bits=word)
    q[100 - 20] = T35 + 1                        # 19
    assert R.video_id(q)['vid_x'] != 100
    q[100 - 20] = T35                            # a pixel of exactly T is not above it
    assert R.video_id(q)['vid_x'] == 100


# ---- the cell sums ------------------------------------------------------------------------------
def test_cell_sum_tie_reads_zero():
    p = R.ideal_cc(339, 0xC1, 0x79)
    c = R.cc_centre(339, 1)                      # bit 1 of 0xC1: a zero
    p[c - 4:c + 5] = T25
    assert R.captions(p)['cc'] == (0xC1, 0x79)
    p[c + 4] = T25 + 1
    rec = R.captions(p)
    assert rec['cc'] == (0xC3, 0x79) and rec['cc_state'] == CHECK
    word = R.vid_word(0x152E)
    p = R.ideal_vid(100, word)
    c = 100 + 16 + 32 * 21                       # the last CRC bit
    p[c - 4:c + 5] = T35
    assert R.video_id(p)['vid_bits'] == word & ~1
    p[c - 4] = T35 + 1
    assert R.video_id(p)['vid_bits'] == word | 1


# ---- the white flag -----------------------------------------------------------------------------
@pytest.mark.parametrize('count,flag', [(0, 0), (340, 0), (341, 1), (680, 1)])
def test_white_count(count, flag):
    assert R.white_flag(R.ideal_white(count)) == dict(white_count=count, white_flag=flag)


def test_white_threshold_and_window():
    assert R.white_flag(R.ideal_white(680, hi=T50))['white_count'] == 0
    assert R.white_flag(R.ideal_white(680, hi=T50 + 1))['white_count'] == 680
    p = R.blank_row()
    p[:100] = p[780:] = R.L100                   # outside [100, 780)
    assert R.white_flag(p)['white_count'] == 0


# ---- run-in, constant rows ----------------------------------------------------------------------
@pytest.mark.parametrize('rises,state', [(5, FRAME), (6, OK), (8, OK), (9, FRAME)])
def test_runin_counts(rises, state):
    rec = R.captions(R.ideal_cc(339, 0xC1, 0x79, rises=rises))
    assert rec == dict(cc_state=state, cc_runin=rises, cc_x=339, cc=(0xC1, 0x79))


def test_runin_window_clamped_at_pixel_3():
    # xs = 270: the window [-9, 230) starts at pixel 3 (pixels 0 and 1 are never read)
    p = R.ideal_cc(270, 0xC1, 0x79, rises=7)
    p[2], p[3] = R.L0, R.L50                     # a rise at 3 counts
    assert R.captions(p)['cc_runin'] == 8
    p[2] = R.L50                                 # no rise at 3; pixel 2 itself is no candidate
    assert R.captions(p)['cc_runin'] == 7


@pytest.mark.parametrize('value', [0, 65535])
def test_constant_rows(value):
    rows = np.full((R.ROWS, R.W), value, dtype=np.uint16)
    rec = R.decode_field(rows)
    assert rec == dict(R.NO_FIELD, white_count=680 if value else 0, white_flag=int(value > 0))
    assert R.decode_field(rows[:20]) == R.NO_FIELD and R.decode_field(None) == R.NO_FIELD


# ---- CRC and parity -----------------------------------------------------------------------------
@pytest.mark.parametrize('data', [0, 0x3FFF, 0x152E])
def test_crc_round_trip(data):
    word = R.vid_word(data)
    assert word >> 6 == data and R.vid_crc_reg(R.bits_of(word, 20)) == 0
    assert R.video_id(R.ideal_vid(100, word)) == dict(vid_state=OK, vid_x=100, vid_bits=word)


def test_crc_detects_every_single_bit_flip():
    word = R.vid_word(0x152E)
    for k in range(20):
        bad = word ^ (1 << k)
        assert R.vid_crc_reg(R.bits_of(bad, 20)) != 0
        assert R.video_id(R.ideal_vid(100, bad)) == dict(vid_state=CHECK, vid_x=100, vid_bits=bad)


def test_reference_cells():
    word = R.vid_word(0x152E)
    assert R.video_id(R.ideal_vid(100, word, ref=(1, 1)))['vid_state'] == FRAME
    # (0, 1): the first rise is cell 1's
    rec = R.video_id(R.ideal_vid(100, R.vid_word(0x3FFF), ref=(0, 1)))
    assert rec['vid_x'] == 132 and rec['vid_state'] == FRAME


def test_caption_parity():
    assert R.with_parity(0x41) == 0xC1 and R.with_parity(0x79) == 0x79
    assert R.captions(R.ideal_cc(339, 0xC1, 0x79))['cc_state'] == OK
    for b0, b1 in ((0x41, 0x79), (0xC1, 0xF9), (0x41, 0xF9)):
        rec = R.captions(R.ideal_cc(339, b0, b1))
        assert rec['cc'] == (b0, b1) and rec['cc_state'] == CHECK


def test_frames_layout():
    a = R.ideal_field(white=R.ideal_white(680), cc=R.ideal_cc(300, 0xC1, 0x79), vid=R.ideal_vid(80, R.vid_word(1)))
    b = R.ideal_field(cc=R.ideal_cc(400, 0x79, 0xC1, rises=9))
    recs = R.decode_frames(R.pack_frames([(a, b), (b, a)]))
    assert recs[0][0] == recs[1][1] == R.decode_field(a) and recs[0][1] == recs[1][0] == R.decode_field(b)
    assert recs[0][0]['white_flag'] == 1 and recs[0][1]['cc_state'] == FRAME


# ---- the captures, through the oracle -----------------------------------------------------------
@pytest.mark.parametrize('case', list(R.CASES))
def test_table(case):
    """One read of the case through the oracle: the record the table claims, and the same record
    on the rows + 1, - 1 and with seeded noise in {-1, 0, 1}."""
    c, fa = R.CASES[case], R.facts(case)
    assert fa['outcome'] == 'valid'
    rec = fa['record']
    print(case, rec)
    assert R.matches(rec, c['expect'][0]) == []
    assert fa['robust']
    if not c['lines']:
        # a plain capture: rows 19 and 20 are picture
        assert rec['cc_state'] == ABSENT and rec['vid_state'] != OK and not rec['white_flag']


def test_table_reaches_every_state():
    cc = {R.facts(c)['record']['cc_state'] for c in R.CASES}
    vid = {R.facts(c)['record']['vid_state'] for c in R.CASES}
    white = {R.facts(c)['record']['white_flag'] for c in R.CASES}
    assert cc == vid == {ABSENT, OK, CHECK, FRAME} and white == {0, 1}
