"""ldg_k_final_lines_div: the final resample with tbc_pixel's division kept, which a context
launches when its hz_ire has no usable reciprocal (csrc/divconst.hpp's condition on the divisor:
a significand of all ones).  No supported system has such an hz_ire, so the
dispatch is driven here with one: the double just below a power of two, against the double one
ulp further down, which takes the reciprocal kernel.  The two divisors differ by 1.1e-16
relative, so the two pictures may differ by a rounding tie here and there, never by more than
one level."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASE = 'ntsc_cav_u8_0p2s'


def _picture(native, rf, data, nsamp, fmt, start, hz_ire):
    p = dict(rf.params(), hz_ire=float(hz_ire))
    ctx = native.Context('NTSC', 0, max_reads=2)
    try:
        ctx.set_filters(p, rf.tables)
        ctx.set_capture(data, nsamp, fmt, 0)
        inf = ctx.decode_reads([start], [1.0])[0]
        pic = ctx.debug(0, 40, np.uint16, int(inf.linecount) * 910) if inf.status == 0 else None
        return int(inf.status), pic
    finally:
        ctx.close()


@pytest.mark.gpu
def test_division_kept_when_hz_ire_has_no_reciprocal():
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden
    from ldgpu import native
    from ldgpu.formats import NAME_TO_FMT, samples_in_bytes
    from ldgpu.rfparams import RFTables
    with open(os.path.join(HERE, 'golden', CASE + '.json')) as fh:
        gold = json.load(fh)
    data = make_golden.build_capture(CASE)
    fmt = NAME_TO_FMT[gold['settings']['fmt']]
    nsamp = samples_in_bytes(fmt, len(data))
    start = gold['stage']['readsample']
    rf = RFTables('NTSC')
    compared = 0
    # NTSC's hz_ire is 12,142.9: the powers of two on either side of it
    for top in (16384.0, 8192.0):
        ones = np.nextafter(top, 0.0)                 # significand all ones: the division kernel
        below = np.nextafter(ones, 0.0)               # the reciprocal kernel
        assert not native.divconst_ok(ones) and native.divconst_ok(below)
        sa, a = _picture(native, rf, data, nsamp, fmt, start, ones)
        sb, b = _picture(native, rf, data, nsamp, fmt, start, below)
        print('hz_ire below %g: status %d / %d' % (top, sa, sb))
        assert sa == sb
        if sa != 0:
            continue
        assert a.size == b.size and a.size >= 200 * 910
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        print('  %d of %d pixels differ, max %d; levels %d .. %d' % ((d != 0).sum(), d.size, d.max(), a.min(), a.max()))
        assert d.max() <= 1 and (d != 0).mean() < 1e-3
        assert a.max() - a.min() > 10000              # a picture, not a clamped constant
        compared += 1
    assert compared >= 1
