"""Division by a constant without the divider (csrc/divconst.hpp): the
helper's own header, driven on the host through ldg_div_const, against the IEEE division bit
for bit over the operands each call site can see.  No GPU.

Sites: u16_to_ire_of and clp1_v in the default 2D comb (div_const_nz: finite operands, no -0),
the comb's I / Q scaling, tbc_pixel and burst_line's statistics -- the means and the variance
over 40 and the level and deviation over hz_ire (div_const: any operand, +-0, +-inf and NaN
included)."""
import numpy as np
import pytest

from ldgpu import native
from ldgpu.rfparams import RFTables

IRESCALE = 358.4                      # csrc/comb.hip
P_2DRANGE = 45 * IRESCALE
HZ_IRE = {'NTSC': 1700000 / 140.0, 'PAL': 800000 / 100.0}
BURST_N = 40.0                        # csrc/tbc.hip burst_line: np.mean / np.std over the 40 burst samples
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan])
NRAND = 10_000_000


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(x, c, guarded):
    x = np.ascontiguousarray(x, dtype=np.float64)
    with np.errstate(all='ignore'):
        want = x / c
    got = native.div_const(x, c, guarded)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (c, guarded, bad.size, x[bad[:5]], got[bad[:5]], want[bad[:5]])
    return x.size


def _random(seed, n=NRAND):
    """Doubles of magnitude 2^-40 .. 2^40, both signs, full significands."""
    rng = np.random.default_rng(seed)
    m = 1.0 + rng.random(n)
    e = rng.integers(-40, 40, n)
    return np.ldexp(m, e) * rng.choice([-1.0, 1.0], n)


def test_constants_meet_the_significand_condition():
    assert HZ_IRE['NTSC'] == RFTables('NTSC').params()['hz_ire']
    assert HZ_IRE['PAL'] == RFTables('PAL').params()['hz_ire']
    for c in (IRESCALE, P_2DRANGE, HZ_IRE['NTSC'], HZ_IRE['PAL'], BURST_N, 1600000 / 143.0):
        assert native.divconst_ok(c), c
    # what the condition excludes: a significand of all ones, zero, subnormals, inf and NaN
    for c in (np.nextafter(2.0, 0.0), -np.nextafter(1024.0, 0.0), 0.0, 5e-324, np.inf, np.nan):
        assert not native.divconst_ok(c), c
    with pytest.raises(ValueError):
        native.div_const(np.ones(4), np.nextafter(2.0, 0.0), True)


def test_u16_to_ire_every_level():
    """(level - 1024) / 358.4 for all 65,536 levels."""
    x = np.arange(65536, dtype=np.float64) - 1024.0
    assert _check(x, IRESCALE, False) == 65536
    _check(x, IRESCALE, True)


def test_clp1_weights():
    """kp / kn = (A - S * .10) / 2 over P_2DRANGE, A = ||c0| - |p0|| + ||cm| - |pm||, S = |c0| + |cm|: every A
    and S that clp0 values within +-512 form, and a fixed grid over those within +-65,535."""
    n = 0
    for grid in (np.arange(0, 1025, dtype=np.float64), np.arange(0, 2 * 65535 + 1, 61, dtype=np.float64)):
        A, S = np.meshgrid(grid, grid, indexing='ij')
        k = A - (S * .10)
        k /= 2
        k = k.ravel()
        assert not (np.signbit(k) & (k == 0)).any()          # no -0 among them
        n += _check(k, P_2DRANGE, False)
        _check(k, P_2DRANGE, True)
    assert n > 5_000_000


@pytest.mark.parametrize('c', [IRESCALE, P_2DRANGE, HZ_IRE['NTSC'], HZ_IRE['PAL'], BURST_N, 1600000 / 143.0])
def test_random_operands_and_specials(c):
    """10^7 fixed-seed doubles, half-integers and tenths, then +-0, +-inf and NaN through the
    guarded form (the comb's I / Q scaling sees -0, tbc_pixel sees NaN and inf samples)."""
    x = _random(int(c * 1000) % 9973)
    _check(x, c, True)
    nz = x[np.isfinite(x) & (x != 0)]
    _check(nz, c, False)
    grid = np.arange(-2_000_000, 2_000_001, dtype=np.float64)
    for y in (grid / 2, grid / 10, grid * .1):
        _check(y, c, True)
        _check(y[y != 0], c, False)
    _check(SPECIALS, c, True)
    # and the unguarded form differs exactly where the header says: -0 (gives +0) and inf (gives NaN)
    got = native.div_const(np.array([-0.0, np.inf]), c, False)
    assert not np.signbit(got[0]) and got[0] == 0 and np.isnan(got[1])


def test_tbc_pixel_operands():
    """(v * wow) - ire0 over hz_ire for demod values around the video band and wow near 1."""
    rng = np.random.default_rng(5)
    for system in ('NTSC', 'PAL'):
        p = RFTables(system).params()
        v = rng.uniform(-2e6, 2e7, NRAND)
        wow = rng.uniform(.97, 1.03, NRAND)
        _check((v * wow) - p['ire0'], p['hz_ire'], True)


def test_burst_statistics_operands():
    """burst_line (burst_lines, burst_field): m = sum(ba) / 40, m2 = sum(ba - m) / 40, the variance
    sum((ba - m - m2)^2) / 40, then lv / hzs and sd / hzs.  ba: 40 samples of the burst channel
    times wow -- a band-passed demod, so within about +-3e7 Hz and often far smaller; a NaN or
    inf sample makes the sums NaN or inf, an all-zero window makes them +0."""
    rng = np.random.default_rng(40)
    hzs = HZ_IRE['NTSC']
    specials = np.array([0.0, np.nan, np.inf, -np.inf])
    n = 0
    for scale in (3e7, 2e6, 3e4, 40.0):
        ba = rng.uniform(-scale, scale, (250_000, 40)) * rng.uniform(.97, 1.03, (250_000, 1))
        sm = 0.0 + ba.sum(axis=1)
        n += _check(sm, BURST_N, True)                          # the mean
        v = ba - (sm / 40.0)[:, None]
        s2 = 0.0 + v.sum(axis=1)
        _check(s2, BURST_N, True)                               # the mean of the deviations (rounding residue)
        d = v - (s2 / 40.0)[:, None]
        var = 0.0 + (d * d).sum(axis=1)                         # up to 40 * (6e7)^2 = 1.4e17 > 2^55
        _check(var, BURST_N, True)
        sd = np.sqrt(var / 40.0)
        lv = np.abs(v).max(axis=1).astype(np.float32).astype(np.float64)      # the level goes through float32
        _check(sd, hzs, True)
        _check(lv, hzs, True)
    assert n == 1_000_000
    # sums of squares over the whole range the variance can take, to 2^57
    m = 1.0 + rng.random(NRAND)
    _check(np.ldexp(m, rng.integers(-20, 57, NRAND)), BURST_N, True)
    # float32 levels and deviations over their range, and the special sums
    lv = np.ldexp(1.0 + rng.random(2_000_000), rng.integers(-10, 26, 2_000_000)).astype(np.float32).astype(np.float64)
    _check(lv, hzs, True)
    _check(specials, BURST_N, True)
    _check(specials, hzs, True)
