"""The Philips code cases of tests/vbi_cases.py do what their table claims, in the oracle (CPU).

test_vbi_gpu.py holds ldg_k_philips and the decode loop to the oracle on these captures; it says
something only while each capture still drives the oracle down the branch it was built for, and
while the oracle's reading of it does not hang on the last bits of the demod.  Here, per case: the
three lines' codes and crossing counts and the vbi dict are the table's, and the same codes and
counts come out of the demod shifted by +-1e-6 of its full scale and with noise of that size
(the GPU demod is held to 1e-9).  Over the table: every crossing-count class and every
interpretation branch on both systems.  For the whole captures: the oracle's field log shows the
events each was built for.  Each read is decoded once per process (vbi_cases.facts).
"""
import numpy as np
import pytest

import vbi_cases as V


@pytest.mark.parametrize('case', list(V.CASES))
def test_case_does_what_it_claims(case):
    e, got = V.CASES[case]['expect'][0], V.facts(case)
    print(case, got)
    assert got['outcome'] == e['outcome']
    assert got['codes'] == e['codes'], got['codes']
    assert got['n'] == e['n'], got['n']
    assert got['vbi'] == e['vbi'], got['vbi']
    # the read is far from the `IndexError` exits: every search stays inside the demod
    assert all(2000 < x < V.READLEN - 4000 for x in got['linelocs'])
    # the gap check never decides: with 24 crossings every gap lies inside 1.85..2.15 us already
    for n, g in zip(got['n'], got['gaps']):
        assert n != 24 or 1.85 < g[0] <= g[1] < 2.15, got['gaps']


@pytest.mark.parametrize('case', list(V.CASES))
def test_case_is_robust(case):
    """The robustness condition, for every case of the table (none is exempt)."""
    assert V.facts(case)['robust']


@pytest.mark.parametrize('system', ['NTSC', 'PAL'])
def test_table_covers_every_branch(system):
    """Per system: 0, fewer than 24, 24 and more than 24 crossings; a line that decodes to None; minutes,
    picture number, seconds with the second nibble >= 10 and < 10, both status codes, 0x87FFFF, and a code
    that takes no branch; a negative decoded value; the later of two codes of a kind winning."""
    fa = [V.facts(case) for case, c in V.CASES.items() if c['system'] == system]
    seen = set().union(*[V.branches(f) for f in fa])
    assert seen >= {'n0', 'n<24', 'n24', 'n>24', 'none', 'minutes', 'framenr', 'seconds<10', 'status_8dc',
                    'status_8ba', '87ffff', 'other'}, seen
    assert any(v < 0 for f in fa for v in f['vbi'].values())
    if system == 'NTSC':
        assert 'seconds>=10' in seen
        assert 7 <= len(fa) <= 30
        codes = {c for f in fa for c in f['codes'] if c}
        # hours 0, 1, 9; the `& 7` mask on 0xF8, 0xFF, 0xF0; every nibble value on a decoded line
        assert {c[1] for c in codes if c[0] == 'F' and c[2] == 'D'} >= {'0', '1', '9'}
        assert {c[1] for c in codes if c[0] == 'F' and c[2] != 'D'} >= {'8', 'F', '0'}
        assert {ch for c in codes for ch in c} == set('0123456789ABCDEF')
        # a line valid between two that are not, and a later code overriding an earlier one of its kind
        assert any(f['codes'][0] is None and f['codes'][1] and f['codes'][2] is None for f in fa)
        assert V.facts('later_pic')['vbi']['framenr'] == 347 and V.facts('later_status')['vbi']['status'] == 0x8BA333


@pytest.mark.parametrize('case', ['edit_part', 'delay', 'p_counts'])
def test_damage_leaves_the_rest_alone(case):
    """The composite differs from the undamaged capture's (same words) only on the damaged code lines and
    inside the edits, and the capture's bytes are the same up to the first of them.  (Not after it: the FM
    phase carries the integral of everything before, so one changed line moves every later sample.)"""
    c = V.CASES[case]
    g, ref = V.generator(c), V.generator(c, lines=False)
    start = c['reads'][0]
    n = np.arange(start, start + 200000, dtype=np.int64)
    a, b = g._ire(n), ref._ire(n)
    la = n / g.spl + g.t0_lines
    touched = np.zeros(n.size, dtype=bool)
    for (k, fld, j) in c['lines']:
        touched |= np.floor(la) == k * g.p['lines'] + g.p['code_lines'][fld][j]
    for line, dur, _ in c['edits']:
        touched |= (la >= line) & (la < line + dur)
    assert touched.any() and not np.array_equal(a[touched], b[touched])
    assert np.array_equal(a[~touched], b[~touched])
    first = int(n[np.nonzero(touched)[0][0]])
    x, y = V.build(case), V.build(case, lines=False)
    assert np.array_equal(x[:first - 64], y[:first - 64]) and not np.array_equal(x[first:first + 4000], y[first:first + 4000])
    if c['dropouts']:
        d0, dn = c['dropouts'][0]
        assert abs(int(x[d0:d0 + dn].astype(np.int64).mean()) - 128) <= 3      # the carrier is gone there


def _merged(o):
    return [m['vbi'] for m in o['meta']]


def whole_events(name):
    """The events of the listed kind that the oracle's decode of a whole capture shows."""
    o = V.oracle_whole(name)
    ev = set()
    fl, vb = o['fields'], _merged(o)
    if o['crashed']:
        ev.add('TypeError')
    if any(v['framenr'] is None and not v['isclv'] for v in vb):
        ev.add('merged framenr None')
    for a, b in zip(fl, fl[1:]):
        if a['valid'] and b['valid'] and a['istop'] and a['vbi']['framenr'] is None and b['vbi']['framenr'] is not None:
            ev.add('codes in the second field only')
        if a['valid'] and b['valid'] and a['istop'] and None not in (a['vbi']['minutes'], b['vbi']['minutes']) and \
                a['vbi']['minutes'] != b['vbi']['minutes']:
            ev.add('fields disagree on minutes')
    valid = [f for f in fl if f['valid']]
    for a, b, c in zip(valid, valid[2:], valid[4:]):
        if a['vbi']['framenr'] is not None and b['vbi']['framenr'] is None and b['mtf'] == c['mtf']:
            ev.add('MTF level held')
    mtfs = [f['mtf'] for f in valid]
    if any(abs(x - y) > .1 for x, y in zip(mtfs, mtfs[1:])):
        ev.add('MTF re-read')
    if any(len(m['fields']) >= 6 for m in o['meta'][1:]):
        ev.add('frames dropped by the re-read')
    if any(v['framenr'] is not None and v['framenr'] < 0 for v in vb):
        ev.add('negative merged framenr')
    return ev


WHOLE_EVENTS = {
    'cav_gaps': {'merged framenr None', 'codes in the second field only', 'MTF level held'},
    'cav_jump': {'MTF re-read', 'frames dropped by the re-read'},
    'clv_odd': {'negative merged framenr', 'fields disagree on minutes'},
    'clv_no_minutes': {'TypeError'},
    'cav_leadout': {'TypeError'},
}


@pytest.mark.parametrize('name', list(V.WHOLE))
def test_whole_capture_shows_its_events(name):
    """The oracle's decode of each whole capture shows what test_vbi_gpu.py's docstrings say of it; the two
    crash captures raise TypeError in mergevbi after two frames."""
    o = V.oracle_whole(name)
    ev = whole_events(name)
    print(name, sorted(ev), [v['framenr'] for v in _merged(o)])
    assert ev >= WHOLE_EVENTS[name], ev
    if name in V.CRASHES:
        assert "'NoneType' and 'int'" in o['crashed'] and len(o['frames']) == 2
    else:
        assert not o['crashed'] and len(o['frames']) >= 5
    if name == 'clv_odd':
        assert [v['framenr'] for v in _merged(o)][2:4] == [-2205, 9204]
    if name == 'cav_jump':
        assert [v['framenr'] for v in _merged(o)][:4] == [201, 202, 205, 206]
