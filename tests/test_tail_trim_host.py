"""The tail plan of a read and the audio guard's bound, on the CPU.

Past a read's video cut the demod also drops demod_05 and, where the cut allows it, the
audio carrier slices, audio phase 1 of those blocks and audio phase 2's last block
(csrc/tail.hpp).  ldg_tail_plan and ldg_audio_reach run the same header on the host:

  * the plan against a restatement of the reference's audio phase 2 block loop
    (lddecode_core.py:348-371, oracle/demod.py audio_phase2): what every block reads and
    which block's value every output keeps;
  * the guard's span against the samples the oracle's downscale_audio really takes.
"""
import json
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

BLOCKLEN, BLOCKCUT, BLOCKSTEP, READLEN = 16384, 1024, 15328, 1000000
NTSC_CUT, PAL_CUT = 740000, 880000


def geometry(start):
    """A read's geometry from its start (lddecode_core.py:373-385, oracle block_starts)."""
    end = int(start + READLEN) + 1
    s0 = start - BLOCKCUT if start > BLOCKCUT else 0
    return sized(end - s0 + 1)


def sized(n_out):
    n_audio = (n_out - 1) // 16 + 1
    return n_out, n_audio, n_audio // 4


def phase2_blocks(n_in, n_out):
    """audio_phase2's blocks in the reference's order: [(first sample read, one past the last
    read)], and owner[o] = the block whose value output o keeps (later writes win)."""
    skip, fdiv2 = 64, 4
    jump = BLOCKLEN - skip * fdiv2
    per = BLOCKLEN // fdiv2
    owner = np.full(n_out, -1)
    blocks = [(0, BLOCKLEN)]
    owner[:per] = 0
    pos = per
    for s in range(jump, n_in - jump, jump):
        m = per - skip
        owner[pos:pos + m] = len(blocks)
        blocks.append((s, s + BLOCKLEN))
        pos += m
    s = n_in - BLOCKLEN - 1
    owner[n_out - (per - skip):] = len(blocks)
    blocks.append((s, s + BLOCKLEN))
    return blocks, owner


READS = ([geometry(s) for s in (385743, 5000, 1025, 1024, 500, 0)]            # full; clipped at the capture's start
         + [sized(n) for n in (1001042, 700000, 300000, 131072, 70001, 20000, 15393)])   # the largest; short ones
CUTS = [0, NTSC_CUT, PAL_CUT, 200000, 40000, 742976, 742977, 1]


@pytest.mark.parametrize('vcut', CUTS)
def test_tail_plan_against_the_block_loop(vcut):
    from ldgpu import native
    engaged = 0
    for n_out, n_audio, n_audio2 in READS:
        acut1, acut2, live2, live1, live05 = native.tail_plan(n_out, n_audio, n_audio2, vcut)
        n_blocks = -(-(n_out - 1) // BLOCKSTEP)
        assert live05 == sum(1 for b in range(n_blocks) if not (vcut > 0 and b * BLOCKSTEP >= vcut))
        assert (acut1 is None) == (acut2 is None)
        if n_audio - BLOCKLEN - 1 < 0 or n_audio2 - 4032 <= 0:
            # the reference's last block starts before the read or serves all of it: never trimmed
            assert acut2 is None and live1 == n_blocks
            continue
        blocks, owner = phase2_blocks(n_audio, n_audio2)
        assert (owner >= 0).all()
        last_only = int(np.flatnonzero(owner == len(blocks) - 1)[0])     # first output only the last block serves
        if vcut == 0 or -(-vcut // 64) > last_only:
            # no cut, or the video below the cut can need audio the last block serves: all of it stays
            assert acut2 is None and live2 == len(blocks) and live1 == n_blocks, (n_out, vcut)
            continue
        engaged += 1
        assert acut2 == last_only and -(-vcut // 64) <= acut2
        live = list(range(len(blocks) - 1))                              # all but the last block
        assert live2 == len(live)
        assert set(owner[:acut2].tolist()) <= set(live)                  # every output < acut2 comes from a live block
        assert (owner[acut2:] == len(blocks) - 1).all()                  # and the dead block serves nothing else
        assert max(blocks[j][1] for j in live) == acut1                  # every sample a live block reads is < acut1
        # demod block b keeps the audio-1 samples [off / 16, (off + copylen) / 16)
        alive = [b for b in range(n_blocks) if b * BLOCKSTEP // 16 < acut1]
        assert live1 == len(alive) and alive == list(range(len(alive)))
    if vcut in (NTSC_CUT, 200000, 40000, 742976):
        assert engaged > 0
    if vcut in (0, PAL_CUT):
        assert engaged == 0


def test_default_cuts():
    """The figures DESIGN.md quotes for a steady-state read: NTSC trims 17 blocks' demod_05, 15
    blocks' audio slices and one of four phase-2 blocks; PAL's cut lies past the last block's
    first output, so PAL keeps all its audio."""
    from ldgpu import native
    n = geometry(385743)
    assert n == (1001026, 62565, 15641)
    assert native.tail_plan(*n, NTSC_CUT) == (48640, 11609, 3, 51, 49)
    assert native.tail_plan(*n, PAL_CUT) == (None, None, 4, 66, 58)
    assert native.tail_plan(*n, 0) == (None, None, 4, 66, 66)


class Recorder:
    """An audio channel that records the indices downscale_audio reads."""

    def __init__(self):
        self.idx = []

    def __getitem__(self, i):
        self.idx.append(int(i))
        return 0.0


_FIELDS = {}


def golden_field(case):
    """(rf, line locations, linecount) of the golden case's first valid field, by the oracle."""
    if case not in _FIELDS:
        sys.path.insert(0, os.path.join(HERE, 'golden'))
        import make_golden
        from oracle.capture import FMT_BY_EXT, Capture
        from oracle.demod import RFDemod
        from oracle.field import FieldNTSC, FieldPAL
        with open(os.path.join(HERE, 'golden', case + '.json')) as fh:
            gold = json.load(fh)
        c = make_golden.CASES[case]
        rf = RFDemod(system=c['system'])
        cap = Capture(make_golden.build_capture(case), FMT_BY_EXT[c['fmt']])
        raw = rf.demod(cap, gold['stage']['readsample'], READLEN, gold['stage']['mtf_level'])
        f = (FieldNTSC if c['system'] == 'NTSC' else FieldPAL)(rf, raw, 0, audio_offset=0)
        assert f.valid and [float(x) for x in f.linelocs[:12]] == gold['stage']['linelocs']
        _FIELDS[case] = (rf, np.array(f.linelocs, dtype=np.float64), int(f.linecount))
    return _FIELDS[case]


@pytest.mark.parametrize('case', ['ntsc_clv_u8_0p2s', 'ntsc_cav_u8_mid_0p2s', 'pal_clv_u8_0p2s'])
def test_audio_guard_bound(case):
    """The span the guard tests (ldg_audio_reach) holds every sample downscale_audio takes, and
    its top is within two lines of the highest one taken (a guard that always fired would
    hold them too): the golden field's line locations, wow-stretched variants of them
    (tests/test_timebase.py's range: the two speed components of make_golden.wow, up to
    0.6 % + 0.4 %) and carried-in time offsets across +-1/48000 s."""
    from ldgpu import native
    from oracle.field import downscale_audio
    rf, lines, lc = golden_field(case)
    srf = types.SimpleNamespace(SysParams=rf.SysParams, linelen=rf.linelen)
    rng = np.random.default_rng(20)
    variants = [lines]
    k = np.arange(lines.size - 1)
    for _ in range(6):
        a1, a2 = rng.uniform(0, 0.006), rng.uniform(0, 0.004)
        p1, p2 = rng.uniform(0, 2 * np.pi, 2)
        speed = 1 + a1 * np.sin(2 * np.pi * k / 37.3 + p1) + a2 * np.sin(2 * np.pi * k / (1.7 * (lc + 0.5)) + p2)
        variants.append(np.concatenate(([lines[0]], lines[0] + np.cumsum(np.diff(lines) * speed))))
    gap = 1 / 48000.0
    worst = 0
    for ll in variants:
        lo, hi = native.audio_reach(ll, lc, rf.linelen)
        assert 0 <= lo <= hi
        for off in np.linspace(-gap, gap, 9):
            au = {'audio_left': Recorder(), 'audio_right': Recorder()}
            downscale_audio(au, ll.tolist(), srf, lc, timeoffset=float(off))
            idx = au['audio_left'].idx
            assert idx == au['audio_right'].idx and len(idx) > 700
            assert int(lo / 64) <= min(idx) and max(idx) <= int(hi / 64)
            assert int(hi / 64) - max(idx) <= 2 * rf.linelen / 64
            worst = max(worst, int(hi / 64) - max(idx))
    print('%s: the bound lies up to %d audio samples above the highest one read' % (case, worst))
    if case == 'ntsc_clv_u8_0p2s':
        # a steady-state read (the case's second) at the default cut is not redone: its span ends below 64 acut2
        acut2 = native.tail_plan(1001026, 62565, 15641, NTSC_CUT)[1]
        assert native.audio_reach(lines, lc, rf.linelen)[1] < 64 * acut2


def test_audio_guard_rejects_what_would_wrap():
    """A negative position (Python's negative indexing would read the read's tail) and a NaN
    both put the span outside [0, 64 acut2)."""
    from ldgpu import native
    ll = np.arange(270) * 2542.0 - 100.0
    assert native.audio_reach(ll, 262, 2542)[0] < 0
    ll = np.arange(270) * 2542.0 + 30000
    ll[100] = np.nan
    lo, hi = native.audio_reach(ll, 262, 2542)
    assert not (lo >= 0) and not (hi < 64 * 11609)
