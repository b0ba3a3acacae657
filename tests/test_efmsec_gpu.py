"""The EFM data sectors on the GPU (csrc/efmsec.hip) against the numpy restatement of the
build-defined rule (tests/efmsec_ref.py), byte for byte: the bytes and
their erasure flags, sector starts, records, user data, whole sectors and every counter -- on the
shared 605-frame stream clean, under an F3 burst the product code repairs and under the first it
does not, and on the stage-level cases; independence of how the stream is cut, through
ldg_efmdec_feed (run lengths) and ldg_efmsec_feed (bytes); the EFM decode's own outputs with and
without the stage; efm_decode.py --data and lddecode.py --efm-data end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import efmdec_ref as R
import efmsec_ref as S
from ldgpu import efmdec, efmsec, native

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOL = os.path.join(ROOT, 'ld-decode_amd', 'efm_decode.py')
DECODE = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
ARRAYS = ('starts', 'records', 'data', 'sectors')
_ctx = []
_ref = {}


def context():
    if not _ctx:
        _ctx.append(native.Context('NTSC', 0, max_reads=1))
    return _ctx[0]


def teardown_module(module):
    for c in _ctx:
        c.close()
    _ctx.clear()


def bursts():
    """The F3 bursts at frame 150: none, one the product code repairs, the first it does not."""
    return {'clean': 0, 'burst18': 18, 'failing': S.first_failing(150)}


def reference(name):
    """(run lengths, the restatement's sector result, its EFM decode), computed once."""
    if name not in _ref:
        rl = S.stream_rl(bursts()[name])
        _ref[name] = (rl, S.decode(rl), R.decode(rl))
    return _ref[name]


def check(got, ref, what, arrays=ARRAYS):
    for k in arrays:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (what, k, int(np.count_nonzero(got[k] != ref[k])))
    for k in efmsec.COUNTERS:
        assert got['counters'][k] == ref['counters'][k], (what, k, got['counters'][k], ref['counters'][k])


def test_record_layout_matches_the_restatement():
    assert native.EFMSEC_REC == S.REC and native.EFMSEC_REC.itemsize == 16
    assert efmsec.COUNTERS == S.COUNTERS


@pytest.mark.parametrize('name', ['clean', 'burst18', 'failing'])
def test_parity_with_the_restatement(name):
    rl, ref, _ = reference(name)
    pcm, got = efmsec.decode(context(), rl, keep=True)
    print(name, got['counters'], got['records']['status'], got['records']['rounds'])
    check(got, ref, name, ARRAYS + ('bytes', 'erased'))
    st = ref['records']['status']
    if name == 'clean':
        assert np.all(st == S.GOOD) and np.array_equal(got['data'], S.stream_bytes()[1])
    if name == 'burst18':
        assert np.all(st <= S.CORRECTED) and (st == S.CORRECTED).any() and np.array_equal(got['data'], S.stream_bytes()[1])
        assert ref['erased'].any()
    if name == 'failing':
        assert (st == S.BAD).any()


@pytest.mark.parametrize('name', S.STAGE_CASES)
def test_stage_cases(name):
    by, er, _ = S.stage_case(name)
    ref = S.stage_result(name)
    check(efmsec.decode_bytes(context(), by, er, keep=True), ref, name)
    for chunk in (5000, 777):
        check(efmsec.decode_bytes(context(), by, er, chunk_bytes=chunk, keep=True), ref, (name, chunk))


@pytest.mark.parametrize('chunk', [4096, 1000, 333])
def test_run_length_cuts_do_not_change_the_output(chunk):
    """4096 run lengths hold about 38 frames, 900 bytes: the calls cut the sync search, the CIRC
    carry and every sector many times over."""
    for name in ('burst18', 'failing'):
        rl, ref, dec = reference(name)
        pcm, got = efmsec.decode(context(), rl, chunk_bytes=chunk, keep=True)
        check(got, ref, (name, chunk), ARRAYS + ('bytes', 'erased'))
        assert np.array_equal(pcm['pcm'], dec['pcm']) and np.array_equal(pcm['flags'], dec['flags'])


@pytest.mark.parametrize('chunk', [5000, 777])
def test_byte_cuts_do_not_change_the_output(chunk):
    for name in ('clean', 'failing'):
        _, ref, _ = reference(name)
        got = efmsec.decode_bytes(context(), ref['bytes'], ref['erased'], chunk_bytes=chunk, keep=True)
        check(got, ref, (name, chunk))


def test_the_decode_is_the_same_with_and_without_the_stage():
    rl, _, dec = reference('burst18')
    ctx = context()
    plain = efmdec.decode(ctx, rl, chunk_bytes=1000, keep=True)
    with_stage, _ = efmsec.decode(ctx, rl, chunk_bytes=1000, keep=True)
    again = efmdec.decode(ctx, rl, chunk_bytes=1000, keep=True)            # detached again
    for k in ('pcm', 'flags', 'subcode') + efmdec.PARITY_ARRAYS:
        assert np.array_equal(plain[k], dec[k]), k
        assert np.array_equal(with_stage[k], plain[k]) and np.array_equal(again[k], plain[k]), k
    assert with_stage['counters'] == plain['counters'] == again['counters']
    for k in efmdec.COUNTERS:
        assert plain['counters'][k] == dec['counters'][k], k


def test_refusals():
    ctx = context()
    by, er, _ = S.stage_case('erased172')
    ctx.efmsec_reset()
    info = ctx.efmsec_feed(by, er, final=True)
    assert info['sectors'] == 3 and info['held_bytes'] == 0 and ctx.efmsec_last_info() == info
    with pytest.raises(native.LDGError, match='ended'):
        ctx.efmsec_feed(by, er)
    with pytest.raises(ValueError):
        ctx.efmsec_feed(by, er[:-1])
    ctx.efmsec_reset()
    assert ctx.efmsec_feed(by[:0], er[:0], final=True)['sectors'] == 0


def run(args, **kw):
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=600, **kw)


def test_efm_decode_tool(tmp_path):
    rl, ref, dec = reference('failing')
    src, a, b = str(tmp_path / 'in.efm'), str(tmp_path / 'plain'), str(tmp_path / 'data')
    rl.tofile(src)
    r0 = run([TOOL, '--chunk-bytes', '4096', src, a])
    r1 = run([TOOL, '--chunk-bytes', '4096', '--data', '--stats', src, b])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout[-2000:] + r0.stderr[-2000:] + r1.stdout[-2000:] + r1.stderr[-2000:]
    # without the flag: no new file; with it the PCM is the same and the data the restatement's
    assert not os.path.exists(a + '.efm.data') and not os.path.exists(a + '.efm.data.json')
    assert open(a + '.efm.pcm', 'rb').read() == open(b + '.efm.pcm', 'rb').read() == dec['pcm'].astype('<i2').tobytes()
    assert open(b + '.efm.data', 'rb').read() == ref['data'].tobytes()
    s = json.load(open(b + '.efm.data.json'))
    for k in efmsec.COUNTERS:
        assert s[k] == ref['counters'][k], k
    assert s['first_address'] == [0, 2, 0] or ref['records']['status'][0] >= 2
    assert len(s['bad_sectors']) == ref['counters']['bad'] + ref['counters']['other'] > 0
    assert s['bad_sectors'][0]['start_byte'] == int(ref['starts'][ref['records']['status'] >= 2][0])
    assert s['address_discontinuities'] == 0 and any(k.startswith('efmsec_fix') for k in s['kernels_ms'])
    p0, p1 = json.load(open(a + '.efm.pcm.json')), json.load(open(b + '.efm.pcm.json'))
    for k in efmdec.COUNTERS:
        assert p0[k] == p1[k], k


def test_lddecode_efm_data_switch(tmp_path):
    """Sectors tiled through the EFM channel under a synthetic capture: lddecode.py --efm-data
    writes what the library gives for the .efm it wrote, and the sectors found are the source's."""
    import efm_ref as E
    from ldgpu.synth import make_capture
    x = np.frombuffer(make_capture(int(40e6 * 0.2), 'u8'), dtype=np.uint8).astype(np.float64)
    nf = int(x.size / (588 * E.FS / E.FC)) + 2
    user, sec = S.plain_sectors(14, seed=41)
    by = np.resize(sec.reshape(-1), 24 * (nf - R.LATENCY))
    rl, _, _ = R.encode(S.to_pcm(by), nf)
    w, _ = E.efm_wave(rl.astype(np.int64), x.size, 300.25, 1.0)
    path, out = str(tmp_path / 'disc.u8'), str(tmp_path / 'dig')
    with open(path, 'wb') as fh:
        fh.write(E.pack(x + 12.0 * w, 'u8'))
    r = run([DECODE, '-l', '2', '--efm-data', path, out])
    assert r.returncode == 0 and 'efm-data:' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    for ext in ('.tbc', '.efm', '.efm.json', '.efm.pcm', '.efm.pcm.json', '.efm.data', '.efm.data.json'):
        assert os.path.exists(out + ext), ext
    pcm, got = efmsec.decode(context(), np.fromfile(out + '.efm', dtype=np.uint8))
    assert open(out + '.efm.pcm', 'rb').read() == pcm['pcm'].astype('<i2').tobytes()
    assert open(out + '.efm.data', 'rb').read() == got['data'].tobytes()
    s = json.load(open(out + '.efm.data.json'))
    for k in efmsec.COUNTERS:
        assert s[k] == got['counters'][k], k
    print(got['counters'])
    assert s['good'] >= 2 and s['bad'] == 0 and s['address_discontinuities'] <= 1       # the tiling wraps once at the most
    rows = {bytes(u) for u in user}
    assert all(bytes(d) in rows for d, st in zip(got['data'], got['records']['status']) if st <= S.CORRECTED)
