"""The Philips VBI decode (ldg_k_philips) and what the decode loop does with its values, on the code
lines of tests/vbi_cases.py: damaged trains, unusual bit patterns and well-formed codes the
decoder was not written with in mind (test_vbi_ref.py asserts on the CPU that each capture does in
the oracle what its table entry says, and that no case hangs on the last bits of the demod).

Stage parity: per case one read through the C ABI against the oracle's Field of the same samples;
status, linecode_ok and linecode of the three lines (zeros where a line did not decode) and the six
vbi members exact, everything else at the bars of test_damage_gpu.py (its check_read).

Whole decode: GPUDecoder at batch 3 and 16 against the oracle's decode loop on captures whose codes
go missing, jump, turn negative or make the reference raise: frames and audio within +-1,
metadata exact, and ReferenceCrash after the frames the reference wrote before its TypeError.
"""
import pytest

import vbi_cases as V
from test_damage_gpu import _same_frames, check_read

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', list(V.CASES))
def test_stage_parity(case, gpu_ctx_ntsc, gpu_ctx_pal):
    from ldgpu import native
    c = V.CASES[case]
    data = V.capture(case)
    ctx, _ = gpu_ctx_ntsc if c['system'] == 'NTSC' else gpu_ctx_pal
    ctx.set_capture(data, data.size, 0, 0)
    inf = ctx.decode_reads(c['reads'], [1.0])[0]
    r = V.oracle_read(case)
    f = r.field
    assert inf.status == native.FS_VALID and f.valid
    got = []
    for j, l in enumerate(r.rf.SysParams['philips_codelines']):
        lc = f.linecode[l]
        ok, code = int(inf.linecode_ok[j]), [int(x) for x in inf.linecode[j]]
        got.append(''.join('%X' % x for x in code) if ok else None)
        assert ok == (0 if lc is None else 1), (l, ok, lc)
        assert code == ([0] * 6 if lc is None else [int(x) for x in lc]), (l, code, lc)
    vbi = {}
    for k, v in (('minutes', inf.vbi_minutes), ('seconds', inf.vbi_seconds), ('clvframe', inf.vbi_clvframe),
                 ('framenr', inf.vbi_framenr), ('status', inf.vbi_status)):
        vbi[k] = None if v == native.VBI_NONE else int(v)
        assert vbi[k] == f.vbi[k], (k, vbi[k], f.vbi[k])
        assert f.vbi[k] is None or f.vbi[k] != native.VBI_NONE
    assert int(inf.vbi_isclv) == (1 if f.vbi['isclv'] else 0)
    print('%s: lines %s, vbi %s' % (case, got, {k: v for k, v in vbi.items() if v is not None}))
    # the table's own claims, so that a capture that stopped doing its job fails here too
    e = c['expect'][0]
    assert got == e['codes'] and {k: v for k, v in vbi.items() if v is not None} == \
        {k: v for k, v in e['vbi'].items() if k != 'isclv'}
    check_read(case, e, r, inf, ctx, 0)


def _decode_whole(name, batch):
    """(frames handed to the sink, the exception decode() raised or None, stats)."""
    from ldgpu.decoder import GPUDecoder
    from oracle.capture import FMT_U8
    o = V.oracle_whole(name)
    dec = GPUDecoder(system='NTSC', batch=batch)
    dec.set_capture(o['data'], FMT_U8)
    got, exc = [], None
    try:
        dec.decode(sink=lambda fr, au, meta: got.append((fr.copy(), au.copy(), meta)))
    except Exception as e:           # noqa: BLE001 (the tests assert on its type)
        exc = e
    st = dec.stats
    dec.ctx.close()
    return o, got, exc, st


def _whole(name, batch):
    o, got, exc, st = _decode_whole(name, batch)
    assert exc is None, repr(exc)
    assert not o['crashed'] and len(got) == len(o['frames']) >= 5
    print(_same_frames(name, got, o) + '; batch=%d: reads %d, used %d' % (batch, st['reads'], st['reads_used']))


@pytest.mark.parametrize('batch', [3, 16])
def test_cav_gaps(batch):
    """CAV, no codes in either field of one frame and codes only in the second field of the next.  The
    oracle's field log shows: a frame whose merged metadata has `framenr: None`; a frame whose first field
    has no picture number and whose second has one; the MTF level held over the frame without codes."""
    _whole('cav_gaps', batch)


@pytest.mark.parametrize('batch', [3, 16])
def test_cav_jump(batch):
    """CAV, picture numbers 201, 202, 9000, 204, 205: `abs(newmtf - oldmtf) > .1` twice.  The oracle's field
    log shows: the fields of 204 read at MTF level 0.1 and those of 205 at 0.98 again (the re-read recursion
    forward and back), one readframe call that reads six fields, and frames 9000 and 204 missing from the
    output (201, 202, 205, ...).  The planner predicts 203 after 202 and level 0.98 throughout."""
    _whole('cav_jump', batch)


@pytest.mark.parametrize('batch', [3, 16])
def test_clv_odd(batch):
    """CLV, one frame with seconds nibble 2 next to minutes 0, one whose fields say minutes 0 and 5.  The
    oracle's field log shows: a negative merged frame number (-2205) and a frame whose two fields disagree
    on minutes, the second field's winning (9204)."""
    _whole('clv_odd', batch)


def _crash(name, batch):
    from ldgpu.decoder import ReferenceCrash
    o, got, exc, _ = _decode_whole(name, batch)
    assert "'NoneType' and 'int'" in o['crashed'] and len(o['frames']) == 2
    assert type(exc) is ReferenceCrash, repr(exc)
    assert len(got) == len(o['frames'])
    print(_same_frames(name, got, o))


@pytest.mark.parametrize('batch', [3, 16])
def test_clv_no_minutes(batch):
    """CLV, the minutes lines of both fields of the third frame flat.  The oracle's loop raises TypeError in
    mergevbi (seconds without minutes) after two frames: GPUDecoder.decode raises ReferenceCrash after
    handing its sink those two frames."""
    _crash('clv_no_minutes', batch)


@pytest.mark.parametrize('batch', [3, 16])
def test_cav_leadout(batch):
    """CAV, 0x80EEEE on the second code line of the third frame: read as seconds -86 without minutes, the
    same TypeError after two frames, the same ReferenceCrash after the same two frames."""
    _crash('cav_leadout', batch)
