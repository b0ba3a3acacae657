"""The EFM run-length extraction's definition on the CPU: the numpy
restatement (tests/efm_ref.py) recovers a synthetic EFM stream under an FM carrier, its
edge cases, the host planning in the library against brute force, and the conditioning the
GPU parity tests (tests/test_efm_gpu.py) rely on."""
import numpy as np
import pytest
import scipy.signal as sps

import efm_ref as R
from ldgpu import efm, native

L = R.L


def test_fir_gains():
    """The pass band holds the EFM fundamentals and harmonics, the stop band the NTSC
    analogue audio carriers."""
    h = R.taps()
    assert h.size == 255 and np.allclose(h, h[::-1])
    f = np.concatenate((np.linspace(196e3, 1.4e6, 400), [2.301e6, 2.812e6]))
    g = 20 * np.log10(np.abs(sps.freqz(h, worN=f, fs=R.FS)[1]))
    print('pass band min %.4f dB, 2.301 MHz %.1f dB, 2.812 MHz %.1f dB' % (g[:400].min(), g[400], g[401]))
    # DESIGN.md section 7c states these to the digits shown (-0.02 dB, -82 dB, -66 dB); scipy
    # gives -0.0243, -81.9 and -66.1, so the comparison is at that precision
    assert round(g[:400].min(), 2) >= -0.02 and round(g[:400].max(), 2) <= 0.02
    assert round(g[400]) <= -82 and round(g[401]) <= -66
    assert np.array_equal(efm.taps(), h)


def test_defaults_are_the_sweeps_choice():
    d = native.efm_defaults()
    assert (d['alpha'], d['beta'], d['delta'], d['fs']) == (R.ALPHA, R.BETA, R.DELTA, R.FS)
    assert (R.ALPHA, R.BETA) in R.CANDIDATES
    assert native.EFM_SEG == R.L and native.EFM_CHANNEL_HZ == R.FC


@pytest.mark.parametrize('clk', [0.985, 1.0, 1.015])
def test_restatement_recovers_the_run_lengths(clk):
    """amp 12 LSB under the 80-LSB FM carrier and the two 10-LSB audio tones, sigma 2: no wrong
    run length after the run-in, aligned by time against the true edges; every sync but the
    last opens a 588-bit frame."""
    raw, edges, runs, res = R.fixture('u8', clk)
    wrong, scored, rms = R.score(res, edges, runs)
    print('clock %g: %d wrong of %d, rms timing %.3f samples' % (clk, wrong, scored, rms))
    assert scored > 35000 and wrong == 0
    s = efm.summarise(res['bytes'][R.RUN_IN:], res['segments'])
    assert s['syncs'] > 400 and s['frames_588'] == s['syncs'] - 1
    assert s['run_lengths'] == sum(s['histogram'].values())
    rel = [g['final_P'] / (R.FS / R.FC) * clk for g in res['segments']]
    assert max(abs(r - 1) for r in rel) < 2e-3


def test_constant_input_is_empty():
    res = R.extract(np.full(3 * L // 2, 128.0))
    assert res['bytes'].size == 0 and res['times'].size == 0
    assert [s['emitted'] for s in res['segments']] == [0, 0]
    assert all(s['final_P'] == R.FS / R.FC for s in res['segments'])


@pytest.mark.parametrize('n', [0, 1, 254, 255, 2000, 2683])
def test_short_file_is_empty(n):
    """Shorter than one FIR-plus-baseline span (blocks 1..9 and their taps: 2684 samples):
    no z, no crossing, no error."""
    x = 128 + 50 * np.sin(np.arange(n) * 0.1)
    res = R.extract(x)
    assert res['bytes'].size == 0 and not np.isfinite(res['z']).any()
    assert native.efm_window(0, 1, n) == R.window(0, 1, n)


def test_first_defined_z():
    x = 128 + 50 * np.sin(np.arange(2684) * 0.1)
    z = R.baseline(R.fir_decimate(x, R.taps()))
    assert np.nonzero(np.isfinite(z))[0].tolist() == list(range(320, 384))
    assert not np.isfinite(R.baseline(R.fir_decimate(x[:-1], R.taps()))).any()


def test_each_crossing_is_emitted_once_by_its_own_segment():
    raw, edges, runs, res = R.fixture('u8', 1.0)
    t = res['times']
    assert R.n_segments(R.N_FIX) == 3 and len(res['segments']) == 3
    assert np.all(np.diff(t) >= 0)
    own = [np.count_nonzero((t >= j * L) & (t < (j + 1) * L)) for j in range(3)]
    seg = res['segments']
    # segment 0's first crossing starts its run and emits nothing; nothing is ignored here
    assert [s['emitted'] + s['ignored'] for s in seg] == [own[0] - 1, own[1], own[2]]
    assert np.all(np.diff(res['when']) > 0) and np.isin(res['when'], t).all()
    j = (res['when'] // L).astype(int)
    assert [np.count_nonzero(j == k) for k in range(3)] == [s['emitted'] for s in seg]
    # a segment alone gives the bytes it gives in the whole
    one = R.extract(R.samples(raw, 0), 1, 2)
    assert np.array_equal(one['bytes'], res['bytes'][seg[0]['emitted']:seg[0]['emitted'] + seg[1]['emitted']])


def test_spike_pair_is_ignored():
    _, res = R.spike_fixture()
    _, _, _, clean = R.fixture('u8', 1.0)
    assert [s['ignored'] for s in res['segments']] == [0, 1, 0]
    assert res['times'].size == clean['times'].size + 2
    assert res['bytes'].size == clean['bytes'].size + 1     # the pair's second crossing is a spurious edge


@pytest.mark.parametrize('n', [2684, 300000, L, L + 65536, R.N_FIX, 3 * L + 5, 40 * L + 77])
def test_window_against_brute_force(n):
    nseg = R.n_segments(n)
    ranges = {(0, 1), (0, nseg), (nseg - 1, nseg), (nseg, nseg + 1), (1, 2), (max(nseg - 2, 0), nseg), (2, 2)}
    for a, b in sorted(ranges):
        if a > b:
            continue
        got = native.efm_window(a, b, n)
        want = R.window(a, b, n) if b > a else (0, 0)
        assert got == want, (a, b, n, got, want)
        lo, hi = got
        assert 0 <= lo <= hi <= n and lo % 12 == 0
    with pytest.raises(ValueError):
        native.efm_window(2, 1, n)
    with pytest.raises(ValueError):
        native.efm_window(-1, 1, n)


def test_window_holds_what_a_range_reads():
    """Extracting a segment range from the window alone (placed in a file of zeros) gives the
    range's bytes: nothing outside the window is read."""
    raw, _, _, res = R.fixture('u8', 1.0)
    x = R.samples(raw, 0)
    lo, hi = native.efm_window(1, 2, x.size)
    y = np.zeros_like(x)
    y[lo:hi] = x[lo:hi]
    seg = res['segments']
    a = seg[0]['emitted']
    assert np.array_equal(R.extract(y, 1, 2)['bytes'], res['bytes'][a:a + seg[1]['emitted']])


def test_segment_range():
    n = R.N_FIX
    assert efm.segment_range(0, None, n) == (0, 3)
    assert efm.segment_range(L - 1, L + 1, n) == (0, 2)
    assert efm.segment_range(L, 2 * L, n) == (1, 2)
    assert efm.segment_range(5 * L, None, n) == (3, 3)
    assert efm.segment_range(10, 10, n) == (0, 1)


@pytest.mark.parametrize('fmt,clk', R.FIXTURES + [('spike', 1.0)])
def test_fixture_conditioning(fmt, clk):
    """What the GPU's exact-equality checks rest on: FP64 reordering of a 255-term sum of
    values <= 1e3 moves z by about 3e-11, so no crossing's |z[m-1] - z[m]| and no rounding
    d / P + 0.5 may come within 1e-6 of a tie.  A seed that fails this is replaced."""
    res = R.spike_fixture()[1] if fmt == 'spike' else R.fixture(fmt, clk)[3]
    print('%s %g: min |dz| %.3g, min distance of d/P + 0.5 from an integer %.3g' % (fmt, clk, res['min_dz'], res['min_round']))
    assert res['min_dz'] > 1e-6
    assert res['min_round'] > 1e-6
