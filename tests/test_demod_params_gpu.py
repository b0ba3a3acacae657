"""The demod's arguments across launches (csrc/demod.hip, DemodKargs): the kernel reads the
arguments of its later phases -- the audio filters, the 0.5 MHz and video filters, the channel,
tile and slice bases, the strides and the system constants -- from the launch's kernarg segment
where it uses them.  The hash tests decode once per context and cannot see a stale or shared
argument; here every decode of a context with a history -- other filters, another MTF level,
another capture in another format, a second context of the other system decoding in between, the
profiling span on, a probed read -- must equal a fresh context's decode of the same input bit for
bit: debug channels 0 - 4 (demod, demod_05, expanded sync, expanded burst, PAL pilot), 10 and 11
(the audio) and 41 (the sync peaks), as test_demod_bits_gpu.py reads them, and the records."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NTSC, PAL = 'ntsc_cav_u8_0p2s', 'pal_clv_lds_0p15s'
ODD_OFFSET = 333333


def _gold(case):
    with open(os.path.join(HERE, 'golden', case + '.json')) as fh:
        return json.load(fh)


_CAP = {}


def _capture(case):
    """(bytes, fmt, system, starts, mtf) of a golden case; 'ntsc_s16': the NTSC case's samples as s16."""
    if case not in _CAP:
        sys.path.insert(0, os.path.join(HERE, 'golden'))
        import make_golden
        from ldgpu.formats import NAME_TO_FMT
        src = NTSC if case == 'ntsc_s16' else case
        g = _gold(src)
        data = make_golden.build_capture(src)
        fmt = NAME_TO_FMT[g['settings']['fmt']]
        if case == 'ntsc_s16':
            data = ((np.frombuffer(data, np.uint8).astype(np.int16) - 128) * 200).tobytes()
            fmt = NAME_TO_FMT['s16']
        r0 = g['stage']['readsample']
        _CAP[case] = (data, fmt, g['settings']['system'], [r0, r0 + ODD_OFFSET], float(g['stage']['mtf_level']))
    return _CAP[case]


def _tables(system, variant):
    """variant 0: the system's filters; 1: the audio filters swapped and the sync detector's
    window widened (ldg_set_filters cross-checks the video, 0.5 MHz, burst and pilot filters
    against each other, so those stay)."""
    from ldgpu.rfparams import RFTables
    rf = RFTables(system)
    params, tables = rf.params(), dict(rf.tables)
    if variant:
        tables['audio_lfilt'], tables['audio_rfilt'] = tables['audio_rfilt'], tables['audio_lfilt']
        params['sync_lo'], params['sync_hi'] = float(rf.iretohz(-60)), float(rf.iretohz(-20))
    return params, tables


def _set_capture(ctx, case):
    from ldgpu.formats import samples_in_bytes
    data, fmt, _, _, _ = _capture(case)
    ctx.set_capture(data, samples_in_bytes(fmt, len(data)), fmt, 0)


def _snapshot(ctx, infos, system):
    from ldgpu import native
    out = []
    for slot, inf in enumerate(infos):
        assert inf.status not in (native.FS_EOF, native.FS_MIGRATED, native.FS_PENDING), (slot, inf.status)
        n_out = int(inf.n_out)
        n_audio2 = ((n_out - 1) // 16 + 1) // 4
        h = {'rec': (int(inf.status), int(inf.npeaks), n_out, int(inf.nextfieldoffset))}
        for ch in range(5 if system == 'PAL' else 4):
            h[ch] = ctx.debug(slot, ch, np.float64, n_out).tobytes()
        for ch in (10, 11):
            h[ch] = ctx.debug(slot, ch, np.float64, n_audio2).tobytes()
        h[41] = ctx.debug(slot, 41, np.int32, 2048)[:max(int(inf.npeaks), 0)].tobytes()
        out.append(h)
    return out


def _decode(ctx, case, starts=None, dmtf=0.0):
    _, _, system, s, mtf = _capture(case)
    starts = s if starts is None else starts
    return _snapshot(ctx, ctx.decode_reads(starts, [mtf + dmtf] * len(starts)), system)


def _context(system, variant=0):
    from ldgpu import native
    ctx = native.Context(system, 0, max_reads=2)
    ctx.set_filters(*_tables(system, variant))
    return ctx


_FRESH = {}


def _fresh(case, variant=0, dmtf=0.0, starts=None):
    """A fresh context's decode of (capture, filters, MTF level, starts): computed once, shared."""
    key = (case, variant, dmtf, None if starts is None else tuple(starts))
    if key not in _FRESH:
        ctx = _context(_capture(case)[2], variant)
        try:
            _set_capture(ctx, case)
            _FRESH[key] = _decode(ctx, case, starts, dmtf)
        finally:
            ctx.close()
    return _FRESH[key]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w)
        bad = [k for k in w if g[k] != w[k]]
        assert not bad, '%s: read %d differs from a fresh context in %s' % (what, i, bad)


@pytest.mark.gpu
@pytest.mark.parametrize('case', [NTSC, PAL])
def test_filters_and_mtf_changed(case):
    ctx = _context(_capture(case)[2])
    try:
        _set_capture(ctx, case)
        _same(_decode(ctx, case), _fresh(case), 'first decode')
        _same(_decode(ctx, case, dmtf=0.5), _fresh(case, dmtf=0.5), 'another MTF level')
        ctx.set_filters(*_tables(ctx.system, 1))
        _same(_decode(ctx, case), _fresh(case, variant=1), 'other filters')
        ctx.set_filters(*_tables(ctx.system, 0))
        _same(_decode(ctx, case), _fresh(case), 'the first filters again')
    finally:
        ctx.close()
    # the variants are live: each changes the demod's outputs
    a, b, c = _fresh(case)[0], _fresh(case, dmtf=0.5)[0], _fresh(case, variant=1)[0]
    assert a[0] != b[0] and a[2] != c[2] and a[10] != c[10]


@pytest.mark.gpu
def test_another_capture_in_another_format():
    ctx = _context('NTSC')
    try:
        _set_capture(ctx, NTSC)
        _same(_decode(ctx, NTSC), _fresh(NTSC), 'u8')
        _set_capture(ctx, 'ntsc_s16')
        _same(_decode(ctx, 'ntsc_s16'), _fresh('ntsc_s16'), 's16 after u8')
        _set_capture(ctx, NTSC)
        _same(_decode(ctx, NTSC), _fresh(NTSC), 'u8 after s16')
    finally:
        ctx.close()


@pytest.mark.gpu
def test_two_systems_alternate():
    n, p = _context('NTSC'), _context('PAL')
    try:
        _set_capture(n, NTSC)
        _set_capture(p, PAL)
        ns, ps = _capture(NTSC)[3], _capture(PAL)[3]
        for k in range(2):
            _same(_decode(n, NTSC), _fresh(NTSC), 'NTSC, round %d' % k)
            _same(_decode(p, PAL), _fresh(PAL), 'PAL, round %d' % k)
            _same(_decode(n, NTSC, starts=ns[::-1]), _fresh(NTSC, starts=ns[::-1]), 'NTSC reversed, round %d' % k)
            _same(_decode(p, PAL, starts=ps[::-1]), _fresh(PAL, starts=ps[::-1]), 'PAL reversed, round %d' % k)
    finally:
        n.close()
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', [NTSC, PAL])
def test_profiling_span_and_probed_read(case):
    from ldgpu import native
    _, _, system, starts, mtf = _capture(case)
    ctx = _context(system)
    try:
        _set_capture(ctx, case)
        ctx.profile(True)
        _same(_decode(ctx, case), _fresh(case), 'span on')
        count, ms = ctx.profile_spans()
        assert count >= 1 and ms > 0, 'the span was not recorded'
        ctx.profile(False)
        _same(_decode(ctx, case), _fresh(case), 'span off again')
        # a probed read: the start is a prediction three samples off; the probe moves the read
        # to the sync peak, and what is decoded is the plain decode from the start it reports
        flags = ctx.decode_reads_async([starts[0] + 3, starts[1]], [mtf, mtf], np.arange(2, dtype=np.int32),
                                       full=[native.READ_PROBE, 0])
        infos = ctx.decode_reads_wait()
        assert flags[0] & native.READ_PROBE, 'the read was not probed'
        moved = [int(x.readsample) for x in infos]
        assert moved[1] == starts[1] and abs(moved[0] - starts[0]) < 800
        print('%s: probe moved the read from %d to %d' % (case, starts[0] + 3, moved[0]))
        if any(x.status == native.FS_MIGRATED for x in infos):
            # a park lost to a switched-out workgroup voids the read: decode again, from the moved start
            infos = ctx.decode_reads(moved, [mtf, mtf])
        _same(_snapshot(ctx, infos, system), _fresh(case, starts=moved), 'probed read')
        _same(_decode(ctx, case), _fresh(case), 'after the probe')
    finally:
        ctx.close()
