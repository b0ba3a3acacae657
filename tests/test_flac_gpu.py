"""FLAC-compressed captures on the GPU (csrc/flac.hip, csrc/flac_plan.hpp)
against the Python restatement tests/flac_ref.py: the frame table, the gaps, the counters and the
samples are equal, exactly, on every stream of tests/flac_cases.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flac_cases as K
import flac_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')


# ---- layout (no GPU needed) ---------------------------------------------------------------------
def test_flac_layout_matches_header(tmp_path):
    """The ctypes mirrors of the ldg_flac_* structs == the C compiler's view of include/ldgpu.h."""
    from ldgpu import native
    structs = (('ldg_flac_info', native.FlacInfo, 'LDG_FLAC_INFO_SIZE'),
               ('ldg_flac_counters', native.FlacCounters, 'LDG_FLAC_COUNTERS_SIZE'))
    body = ''
    for name, cls, macro in structs:
        body += 'printf(" %%zu %%d", sizeof(%s), %s);' % (name, macro)
        body += ''.join('printf(" %%zu", offsetof(%s, %s));' % (name, k) for k, _ in cls._fields_)
    body += 'printf(" %zu %d", sizeof(ldg_flac_frame), LDG_FLAC_FRAME_SIZE);'
    body += ''.join('printf(" %%zu", offsetof(ldg_flac_frame, %s));' % k
                    for k in ('offset', 'bytes', 'position', 'block_size', 'state'))
    body += 'printf(" %d %d %d %d %d\\n", LDG_FLAC_KEPT, LDG_FLAC_NESTED, LDG_FLAC_MISPLACED, LDG_FLAC_NATIVE, LDG_FLAC_OGG);'
    src = tmp_path / 'fl.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ldgpu.h"\nint main(void){' + body + 'return 0;}')
    exe = tmp_path / 'fl'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    want = []
    for name, cls, macro in structs:
        want += [C.sizeof(cls), getattr(native, macro[4:])] + [getattr(cls, k).offset for k, _ in cls._fields_]
    fr = native.FLAC_FRAME
    want += [fr.itemsize, native.FLAC_FRAME_SIZE] + [fr.fields[k][1] for k in fr.names]
    want += [native.FLAC_KEPT, native.FLAC_NESTED, native.FLAC_MISPLACED, 0, 1]
    assert got == want
    assert (F.KEPT, F.NESTED, F.MISPLACED) == (native.FLAC_KEPT, native.FLAC_NESTED, native.FLAC_MISPLACED)
    assert tuple(F.COUNTERS) == tuple(native.FLAC_COUNTERS)
    assert {'ldg_flac_open', 'ldg_flac_index', 'ldg_flac_frames', 'ldg_flac_read', 'ldg_flac_capture',
            'ldg_flac_close'} <= set(native.EXPORTS)


# ---- the device against the restatement ---------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from ldgpu import native
    c = native.Context('NTSC', 0, max_reads=1)
    yield c
    c.close()


_REF = {}


def ref_of(data):
    """The restatement's result for a file, computed once."""
    key = hashlib.md5(data).digest()
    if key not in _REF:
        _REF[key] = F.decode(data)
    return _REF[key]


def check(ctx, data, tmp_path, chunk=0, ext='flac', read=True):
    from ldgpu.flac import FlacFile
    ref = ref_of(data)
    p = tmp_path / ('x.' + ext)
    p.write_bytes(data)
    with FlacFile(ctx, str(p), chunk_bytes=chunk) as f:
        frames, gaps = f.tables()
        print(f.counters)
        assert f.counters == ref['counters']
        assert f.nsamples == ref['n']
        assert [tuple(int(v) for v in r) for r in frames.tolist()] == ref['frames']
        assert [tuple(int(v) for v in g) for g in gaps.tolist()] == ref['gaps']
        assert f.info['md5'] == ref['info']['md5'] and f.info['total_samples'] == ref['info']['total_samples']
        if read and ref['samples'] is not None:
            want = ref['samples']
            got = f.read()
            assert got.dtype == want.dtype and np.array_equal(got, want)
            if len(want) > 10:         # a window that cuts frames at both ends
                a, n = len(want) // 3 + 1, len(want) // 2
                assert np.array_equal(f.read(a, n), want[a:a + n])
    return ref


@pytest.mark.gpu
def test_kinds(ctx, tmp_path):
    st = K.kinds()
    ref = check(ctx, st.native(K.EXTRA), tmp_path)
    assert np.array_equal(ref['samples'], st.truth())


@pytest.mark.gpu
def test_fixed_and_numbers(ctx, tmp_path):
    st = K.fixed()
    assert np.array_equal(check(ctx, st.native(), tmp_path)['samples'], st.truth())
    a, b, c = K.numbers()
    assert check(ctx, a.native(), tmp_path)['gaps'] == [(0, 126 * 16)]
    assert np.array_equal(check(ctx, b.native(), tmp_path)['samples'], b.truth())
    ref = check(ctx, c.native(), tmp_path, read=False)          # a frame at 2^35: the index only
    assert ref['n'] == (1 << 35) + 16


@pytest.mark.gpu
def test_big(ctx, tmp_path):
    st = K.big()
    assert np.array_equal(check(ctx, st.native(), tmp_path)['samples'], st.truth())


@pytest.mark.gpu
@pytest.mark.parametrize('chunk', [256, 4096 + 256, 70144])
def test_chunks(ctx, tmp_path, chunk):
    """The result does not depend on the chunk: frames begin in one chunk and end in a later one."""
    check(ctx, K.kinds().native(K.EXTRA), tmp_path, chunk=chunk)
    check(ctx, K.big().native(), tmp_path, chunk=chunk)
    check(ctx, K.kinds().ogg(payload=4096)[0], tmp_path, chunk=chunk, ext='oga')


@pytest.mark.gpu
def test_adversarial(ctx, tmp_path):
    st = K.adversarial()
    ref = check(ctx, st.native(), tmp_path)
    assert ref['counters']['nested'] == 1 and np.array_equal(ref['samples'], st.truth())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['bitflip', 'removed', 'junk', 'cut', 'zeros', 'metadata_only'])
def test_damage(ctx, tmp_path, name):
    data, truth, gaps, kept = K.damaged()[name]
    ref = check(ctx, data, tmp_path)
    assert ref['gaps'] == gaps and ref['counters']['kept'] == kept and np.array_equal(ref['samples'], truth)


@pytest.mark.gpu
def test_ogg(ctx, tmp_path):
    for st in (K.kinds(), K.fixed()):
        ref = check(ctx, st.ogg(payload=4096)[0], tmp_path, ext='ldf')
        assert np.array_equal(ref['samples'], st.truth()) and ref['counters']['lost_bytes'] == 0
    st = K.small_packets()
    for kw in (dict(payload=600), dict(payload=600, foreign=0x77), dict(payload=600, header_count=0),
               dict(payload=255, flush_each=True)):
        assert np.array_equal(check(ctx, st.ogg(**kw)[0], tmp_path, ext='oga')['samples'], st.truth())
    wide = K.wide_packet()
    data, pages = wide.ogg(payload=255 * 255)
    assert any(p[26] == 255 for p in pages)
    assert np.array_equal(check(ctx, data, tmp_path, ext='oga')['samples'], wide.truth())
    # a lost page: one dropped packet and its gap; a lost continuation: the packet is dropped
    data, pages = st.ogg(payload=255, flush_each=True)
    ref = check(ctx, b''.join(pages[:6] + pages[7:]), tmp_path, ext='oga')
    assert ref['gaps'] == [(st.frames[3][0], 16)]
    ref = check(ctx, b''.join(pages[:3] + pages[4:]), tmp_path, ext='oga')
    assert ref['counters']['ogg_broken'] == 1 and ref['gaps'] == [(0, 250)]


@pytest.mark.gpu
def test_eight_bit(ctx, tmp_path):
    st = K.eight()
    ref = check(ctx, st.native(), tmp_path)
    assert ref['samples'].dtype == np.uint8 and np.array_equal(ref['samples'], st.truth())


@pytest.mark.gpu
def test_refusals(ctx, tmp_path):
    from ldgpu import native
    from ldgpu.flac import FlacFile
    cases = dict(K.refusals())
    a, _, _ = K.numbers()
    for name, data in cases.items():
        p = tmp_path / (name + '.flac')
        p.write_bytes(data)
        with pytest.raises(native.LDGError) as e:
            FlacFile(ctx, str(p))
        assert 'ldg_flac_open' in str(e.value) and len(str(e.value)) > 40
    p = tmp_path / 'f8.flac'
    p.write_bytes(F.native_stream(F.streaminfo(16, 32), [f for _, _, f in a.frames]))
    with pytest.raises(native.LDGError) as e:
        FlacFile(ctx, str(p))
    assert 'fixed-block-size' in str(e.value)
    with pytest.raises(native.LDGError):
        FlacFile(ctx, str(tmp_path / 'absent.flac'))
    st = K.fixed()                                              # the context is usable afterwards
    assert np.array_equal(check(ctx, st.native(), tmp_path)['samples'], st.truth())


@pytest.mark.gpu
def test_ldf_unpack(tmp_path):
    import ldf_unpack
    st = K.kinds()
    src = tmp_path / 'k.ldf'
    src.write_bytes(st.ogg(payload=4096)[0])
    assert ldf_unpack.main(['--md5', '--stats', str(src), str(tmp_path / 'k.r16')]) == 0
    assert (tmp_path / 'k.r16').read_bytes() == st.truth().tobytes()
    info = json.load(open(tmp_path / 'k.json'))
    assert info['md5_verdict'] == 'match' and info['nsamples'] == len(st.truth()) and info['gaps'] == []
    assert info['counters']['kept'] == len(st.frames)
    assert ldf_unpack.main(['--start-sample', '1000', '--length', '30001', str(src), str(tmp_path / 'w.r16')]) == 0
    assert (tmp_path / 'w.r16').read_bytes() == st.truth()[1000:31001].tobytes()
    e = K.eight()
    (tmp_path / 'e.flac').write_bytes(e.native())
    assert ldf_unpack.main(['--md5', str(tmp_path / 'e.flac'), str(tmp_path / 'e.u8')]) == 0
    assert (tmp_path / 'e.u8').read_bytes() == e.truth().tobytes()
    assert json.load(open(tmp_path / 'e.json'))['md5_verdict'] == 'match'


# ---- lddecode.py end to end ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def e2e(tmp_path_factory):
    """The capture of golden case ntsc_cav_s16_0p15s as .r16, native FLAC and Ogg FLAC."""
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden
    d = tmp_path_factory.mktemp('flac_e2e')
    data = bytes(make_golden.build_capture('ntsc_cav_s16_0p15s'))
    s = np.frombuffer(data, dtype='<i2')
    si, frames = F.encode_fast_frames(s, bs=4096, order=2)
    flac = b'fLaC' + F.meta_block(0, si, True) + b''.join(frames)
    (d / 'cap.r16').write_bytes(data)
    (d / 'cap.flac').write_bytes(flac)
    (d / 'cap.ldf').write_bytes(F.ogg_stream(si, frames, payload=4096, crc=False)[0])
    return d


def run_cli(d, src, out, *args):
    r = subprocess.run([sys.executable, CLI, *args, str(d / src), str(d / out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


@pytest.mark.gpu
@pytest.mark.parametrize('args', [(), ('-s', '1', '-l', '2')])
def test_lddecode_flac_equals_r16(e2e, args):
    tag = 'w' if not args else 's'
    run_cli(e2e, 'cap.r16', tag + '_r16', *args)
    for src in ('cap.flac', 'cap.ldf'):
        out = tag + '_' + src[4:]
        run_cli(e2e, src, out, *args)
        for ext in ('.tbc', '.pcm', '.json'):
            assert (e2e / (out + ext)).read_bytes() == (e2e / (tag + '_r16' + ext)).read_bytes(), (src, ext)
    assert (e2e / (tag + '_r16.tbc')).stat().st_size > 0


@pytest.fixture(scope='module')
def cut_capture(tmp_path_factory):
    """The capture tests/test_cli.py seeks and cuts in (0.5 s of a CAV disc from picture 100 with picture
    numbers on the first field of a frame only, which the reference's findframe needs; the golden
    case ntsc_cav_s16_0p15s carries them on both fields and ends findframe in its end-of-capture
    error as a .r16 too), as .u8 and as 8-bit FLAC.  Verbatim frames: the encoder's quickest, and the
    cut reads the same samples whatever the subframes."""
    from ldgpu.synth import make_capture
    d = tmp_path_factory.mktemp('flac_cut')
    data = bytes(make_capture(int(40e6 * 0.5), 'u8', first_frame=100, seed=11, code_fields=(0,)))
    si, frames = F.encode_fast_frames(np.frombuffer(data, dtype=np.uint8), bs=4096, bps=8, order=None)
    (d / 'cap.u8').write_bytes(data)
    (d / 'cap.flac').write_bytes(b'fLaC' + F.meta_block(0, si, True) + b''.join(frames))
    return d


@pytest.mark.gpu
def test_lddecode_flac_cut(cut_capture):
    """-c -S -E on the compressed capture writes the bytes it writes for the raw one."""
    d = cut_capture
    cut = ('-c', '-S', '103', '-E', '106')
    run_cli(d, 'cap.u8', 'c_u8', *cut)
    run_cli(d, 'cap.flac', 'c_flac', *cut)
    want = (d / 'c_u8.r16').read_bytes()
    assert len(want) > 2 * 3 * 1300000                 # three frames and more, int16
    assert (d / 'c_flac.r16').read_bytes() == want
    raw = np.frombuffer((d / 'cap.u8').read_bytes(), dtype=np.uint8).astype('<i2').tobytes()
    assert want in raw                                 # the raw slice itself, as int16


@pytest.mark.gpu
def test_lddecode_flac_refusals_and_notes(e2e, monkeypatch, capsys):
    for extra, env in ((('--efm',), {}), (('--efm-pcm',), {}), (('--efm-data',), {}), (('--epoch-frames', '2'), {}),
                       (('--manifest', str(e2e / 'man.json')), {}), ((), {'WORLD_SIZE': '2'})):
        r = subprocess.run([sys.executable, CLI, *extra, str(e2e / 'cap.ldf'), str(e2e / 'no')], capture_output=True,
                           text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 1 and 'ldf_unpack.py' in r.stdout, (extra, env, r.stdout[-500:], r.stderr[-500:])
        assert not (e2e / 'no.tbc').exists()
    r = run_cli(e2e, 'cap.flac', 'wm', '--window-mb', '64', '-l', '1')
    assert '--window-mb is ignored' in r.stdout
    # device memory too small for the samples: refused with the way out, before anything is allocated
    import lddecode
    from ldgpu import native
    monkeypatch.setattr(native, 'device_memory', lambda device=0: (1 << 20, 1 << 30))
    assert lddecode.main([str(e2e / 'cap.flac'), str(e2e / 'big')]) == 1
    out = capsys.readouterr().out
    assert 'ldf_unpack.py' in out and '-s / -l' in out and not (e2e / 'big.tbc').exists()


@pytest.mark.gpu
def test_scratch_follows_the_file(tmp_path):
    """A context that has read a file of small blocks reads one of the largest blocks next (the decode
    scratch is sized by the file, not by the first file the context saw), and the other way round."""
    from ldgpu import native
    c = native.Context('NTSC', 0, max_reads=1)
    try:
        for st in (K.fixed(), K.big(), K.eight(), K.big()):
            assert np.array_equal(check(c, st.native(), tmp_path)['samples'], st.truth())
    finally:
        c.close()
