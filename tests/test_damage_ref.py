"""The damaged-sync cases of tests/damage.py do what their table claims, in the oracle (CPU).

test_damage_gpu.py holds the HIP field kernels to the oracle on these captures; it says
something only while each capture still drives the oracle down the branch it was built for.
Here each read's claims are asserted (outcome, vsync count, printed lines, new bad lines,
missing VBI, moved nextfieldoffset, peak count against the undamaged read's), and, over the
whole table, that every outcome and every repair / fill path is reached on both systems.
Each read is decoded once per process (damage.facts).
"""
import pytest

import damage as D


@pytest.mark.parametrize('case', list(D.CASES))
def test_case_does_what_it_claims(case):
    c = D.CASES[case]
    for k in range(len(c['reads'])):
        D.check_claims(case, k)
        got = D.facts(case, k)
        print('%s read %d: %s, %d peaks, vsyncs %s, nfo %s, log %s' % (
            case, c['reads'][k], got['outcome'], got['npeaks'], got.get('vsyncs'), got.get('nfo'), got['log']))


@pytest.mark.parametrize('system', ['NTSC', 'PAL'])
def test_table_covers_every_branch(system):
    """Per system: every outcome (no_vsync through both of its exits), a zero vote repaired
    from the next vsync and one from the previous, three or more vsyncs, both log lines,
    and the head, interior and tail fills of compute_linelocs."""
    reads = [D.facts(case, k) for case, c in D.CASES.items() if c['system'] == system for k in range(len(c['reads']))]
    assert 20 <= len(reads) <= 35
    outcomes = {r['outcome'] for r in reads}
    assert outcomes >= {'valid', 'no_vsync', 'short', 'linelocs', 'tbc', 'crash'}, outcomes
    nv = [r['npeaks'] for r in reads if r['outcome'] == 'no_vsync']
    assert min(nv) < 200 <= max(nv), nv
    votes = set().union(*[r.get('votes', set()) for r in reads])
    assert votes == {'next', 'prev'}
    assert max(r.get('nvsync', 0) for r in reads) >= 3
    # three or more vsyncs on a field that decodes, with nextfieldoffset mid-field
    assert any(r['outcome'] == 'valid' and r['nvsync'] >= 3 for r in reads)
    logged = {l for r in reads for l in r['log']}
    assert D.NOVS in logged and any(l.startswith('vsync vote needed') for l in logged), logged
    fills = set().union(*[r.get('fills', set()) for r in reads])
    assert fills == {'head', 'interior', 'tail'}
    # both ways out of `short`: a jump to a real peak, and the 240-line jump
    short = [r for r in reads if r['outcome'] == 'short']
    assert any(D.NOVS in r['log'] for r in short) and any(D.NOVS not in r['log'] for r in short)
    assert any(r['outcome'] == 'valid' and r['framenr'] is None for r in reads)


def test_edits_are_chunk_independent_and_leave_the_rest_alone():
    """An edit changes the composite only inside its span, the same however the capture is
    chunked, and the parent's dropouts still apply."""
    import numpy as np
    from ldgpu.synth import SynthRF
    edits = [(101.25, 0.5, -40.0), (103.0, 0.1, 0.0)]
    g = D.DamagedRF(system='NTSC', edits=edits, **D.BASE)
    ref = SynthRF(system='NTSC', **D.BASE)
    n = np.arange(0, 12000, dtype=np.int64)
    a, b = g._ire(n), ref._ire(n)
    spl = g.spl
    inside = np.zeros(n.size, dtype=bool)
    for line, dur, ire in edits:
        lo, hi = (line - 100) * spl, (line - 100 + dur) * spl
        m = (n >= lo) & (n < hi)
        assert m.any() and np.all(a[m] == ire)
        inside |= m
    assert np.array_equal(a[~inside], b[~inside])
    parts = np.concatenate([g._ire(n[:5000]), g._ire(n[5000:])])
    assert np.array_equal(parts, a)
    d = D.DamagedRF(system='NTSC', edits=edits, dropouts=((3000, 500),), **D.BASE).generate(6000)
    c = D.DamagedRF(system='NTSC', edits=edits, **D.BASE).generate(6000)
    assert np.array_equal(d[:3000], c[:3000]) and not np.array_equal(d[3000:3500], c[3000:3500])
