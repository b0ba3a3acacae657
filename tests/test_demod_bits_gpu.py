"""The demod's outputs bit for bit.  tests/golden/demod_bits.json holds
SHA-256 hashes of what the demod kernel, audio phases 1 - 2 and the peak walk leave in HBM for a
few reads of four golden captures, written on an MI355X by the commit the fixture's header
names.  A change to the demod's integer side (addresses, predicates, index math, unpacking)
must reproduce every hash; the hashes are regenerated only when arithmetic is changed on
purpose:

    python tests/test_demod_bits_gpu.py COMMIT        (LDGPU_LIB: the library of that commit)

Per read: the debug channels 0 - 4 (demod, demod_05, expanded sync, expanded burst, PAL
pilot), 10 and 11 (the 625 kHz audio, fed by the carrier slices) and 41 (the sync peaks, fed
by the sync tiles).  Each case is decoded once under the default video cut and once with every
read in the `full` mask.  Under the cut a channel is hashed as far as it is written: the video
channels up to the cut, the audio up to the tail plan's acut2 (native.tail_plan), the sync
channel whole.  The reads start at 0 (the first block keeps its head), at the golden case's
first field read and at an odd offset from it, so the first block, the cut blocks and the last
block's partial wave are all in the hashes, through the u8, s16, .lds and .r30 loaders."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'demod_bits.json')
CASES = ['ntsc_cav_u8_0p2s', 'ntsc_cav_s16_0p15s', 'pal_clv_lds_0p15s', 'pal_cav_r30_0p15s']
MODES = ['cut', 'full']
VIDEO_CUT = {'NTSC': 740000, 'PAL': 880000}           # GPUDecoder's defaults
ODD_OFFSET = 333333


def _golden(case):
    with open(os.path.join(HERE, 'golden', case + '.json')) as fh:
        return json.load(fh)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _decode(ctx, native, starts, mtfs, full):
    slots = np.arange(len(starts), dtype=np.int32)
    flags = [native.READ_FULL if full else 0] * len(starts)
    ctx.decode_reads_async(starts, mtfs, slots, full=flags)
    infos = ctx.decode_reads_wait()
    for _ in range(3):
        # a read whose park was lost to a switched-out workgroup is void: decode it again
        redo = [i for i, x in enumerate(infos) if x.status == native.FS_MIGRATED]
        if not redo:
            break
        ctx.decode_reads_async([starts[i] for i in redo], [mtfs[i] for i in redo], slots[redo],
                               full=[flags[i] for i in redo])
        for i, x in zip(redo, ctx.decode_reads_wait()):
            infos[i] = x
    return infos


def case_hashes(case):
    """{mode: [per read {what: sha256}]} of one golden case on the GPU."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden
    from ldgpu import native
    from ldgpu.formats import NAME_TO_FMT, samples_in_bytes
    from ldgpu.rfparams import RFTables
    gold = _golden(case)
    system = gold['settings']['system']
    data = make_golden.build_capture(case)
    assert hashlib.sha256(data).hexdigest() == gold['capture_sha256']
    r0, mtf = gold['stage']['readsample'], gold['stage']['mtf_level']
    starts = [0, r0, r0 + ODD_OFFSET]
    mtfs = [mtf] * len(starts)
    cut = VIDEO_CUT[system]
    rf = RFTables(system)
    ctx = native.Context(system, 0, max_reads=len(starts))
    out = {}
    try:
        ctx.set_filters(rf.params(), rf.tables)
        fmt = NAME_TO_FMT[gold['settings']['fmt']]
        ctx.set_capture(data, samples_in_bytes(fmt, len(data)), fmt, 0)
        ctx.set_video_cut(cut)
        for mode in MODES:
            full = mode == 'full'
            infos = _decode(ctx, native, starts, mtfs, full)
            reads = []
            for slot, inf in enumerate(infos):
                assert inf.status not in (native.FS_EOF, native.FS_MIGRATED, native.FS_PENDING), (case, mode, slot)
                n_out = int(inf.n_out)
                n_audio = (n_out - 1) // 16 + 1
                n_audio2 = n_audio // 4
                acut2 = None if full else native.tail_plan(n_out, n_audio, n_audio2, cut)[1]
                vlim = n_out if full else min(n_out, cut)
                alim = n_audio2 if acut2 is None else min(acut2, n_audio2)
                h = {'n_out': n_out, 'npeaks': int(inf.npeaks)}
                for ch in range(5 if system == 'PAL' else 4):
                    a = ctx.debug(slot, ch, np.float64, n_out)
                    assert a.size == n_out
                    h[str(ch)] = _sha(a if ch == 2 else a[:vlim])
                for ch in (10, 11):
                    a = ctx.debug(slot, ch, np.float64, n_audio2)
                    assert a.size == n_audio2
                    h[str(ch)] = _sha(a[:alim])
                h['41'] = _sha(ctx.debug(slot, 41, np.int32, 2048)[:max(int(inf.npeaks), 0)])
                reads.append(h)
            out[mode] = reads
    finally:
        ctx.close()
    return out


@pytest.fixture(scope='module')
def fixture_hashes():
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    assert fx['header']['commit'] and 'regenerated only' in fx['header']['note']
    return fx['hashes']


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_demod_outputs_bit_for_bit(case, fixture_hashes):
    got = case_hashes(case)
    want = fixture_hashes[case]
    bad = []
    for mode in MODES:
        assert len(got[mode]) == len(want[mode]) == 3
        for i, (g, w) in enumerate(zip(got[mode], want[mode])):
            assert set(g) == set(w), (mode, i)
            bad += ['%s read %d what %s' % (mode, i, k) for k in sorted(w) if g[k] != w[k]]
    print('%s: %d hashes compared, %d differ' % (case, sum(len(r) for m in MODES for r in want[m]), len(bad)))
    assert not bad, bad


def test_fixture_is_whole():
    """(no GPU) Every case, mode, read and channel has its hash; the PAL cases hold the pilot."""
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    assert sorted(fx['hashes']) == sorted(CASES)
    for case in CASES:
        keys = {'n_out', 'npeaks', '0', '1', '2', '3', '10', '11', '41'} | ({'4'} if case.startswith('pal') else set())
        for mode in MODES:
            reads = fx['hashes'][case][mode]
            assert len(reads) == 3
            for r in reads:
                assert set(r) == keys
                assert all(len(r[k]) == 64 for k in keys - {'n_out', 'npeaks'})
        # the cut is live: under it the video channels are hashed over fewer samples
        assert all(c['0'] != f['0'] for c, f in zip(fx['hashes'][case]['cut'], fx['hashes'][case]['full']))


if __name__ == '__main__':
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'ld-decode_amd')]
    note = ('SHA-256 of the demod debug channels per read (tests/test_demod_bits_gpu.py). Written on an '
            'MI355X by the library of the commit named here; regenerated only when the demod\'s arithmetic '
            'is changed on purpose.')
    fx = {'header': {'commit': sys.argv[1], 'note': note, 'video_cut': VIDEO_CUT, 'odd_offset': ODD_OFFSET},
          'hashes': {case: case_hashes(case) for case in CASES}}
    dst = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(dst, 'w') as fh:
        json.dump(fx, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', dst)
