"""The EFM decode on the GPU (csrc/efmdec.hip) against the numpy restatement of the
build-defined rule (tests/efmdec_ref.py), byte for byte: frame starts,
F3 bytes, C1 and C2 outputs and flags, samples, flags, subcode and every counter, on clean and
damaged streams; chunking; empty inputs; efm_decode.py, the RF-level path through
ldg_efm_extract, and lddecode.py --efm-pcm end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import efm_ref as E
import efmdec_ref as R
from ldgpu import efm, efmdec, native

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOL = os.path.join(ROOT, 'ld-decode_amd', 'efm_decode.py')
DECODE = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
STREAMS = ['clean', 'burst24', 'undetected', 'slip', 'lostsync', 'merged']
ARRAYS = ('starts', 'f3', 'c1', 'c1_flags', 'c2', 'c2_flags', 'pcm', 'flags', 'subcode')
_ctx = []


def context():
    if not _ctx:
        _ctx.append(native.Context('NTSC', 0, max_reads=1))
    return _ctx[0]


def teardown_module(module):
    for c in _ctx:
        c.close()
    _ctx.clear()


def check(got, ref, what):
    for k in ARRAYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (what, k, int(np.count_nonzero(got[k] != ref[k])))
    for k in efmdec.COUNTERS:
        assert got['counters'][k] == ref['counters'][k], (what, k, got['counters'][k], ref['counters'][k])


@pytest.mark.parametrize('name', STREAMS)
def test_parity_with_the_restatement(name):
    ref = R.reference(name)
    got = efmdec.decode(context(), R.stream(name), keep=True)
    print(name, got['counters'])
    check(got, ref, name)
    if name == 'undetected':
        assert ref['counters']['c2_fixed'] > 56 and ref['counters']['c2_failed'] > 0
    if name == 'burst24':
        assert ref['counters']['flagged'] > 0 and ref['counters']['c2_unsolved'] > 0 and ref['counters']['c2_erasure_solved'] > 0


@pytest.mark.parametrize('chunk', [4096, 1000, 333])
def test_chunking_does_not_change_the_output(chunk):
    """4096 bytes hold about 38 frames: the calls cut the sync search, the 111-frame CIRC
    carry and the concealment's neighbours many times over."""
    for name in ('burst24', 'lostsync'):
        check(efmdec.decode(context(), R.stream(name), chunk_bytes=chunk, keep=True), R.reference(name), (name, chunk))


def test_empty_and_syncless_inputs():
    ctx = context()
    got = efmdec.decode(ctx, np.zeros(0, dtype=np.uint8), keep=True)
    assert got['pcm'].shape == (0, 2) and got['subcode'].size == 0 and not any(got['counters'].values())
    rl = np.random.default_rng(3).integers(3, 11, 5000).astype(np.uint8)
    rl[100:102] = 11
    for chunk in (None, 512):
        got = efmdec.decode(ctx, rl, chunk_bytes=chunk, keep=True)
        check(got, R.decode(rl), chunk)
        assert got['counters']['candidates'] == 1 and got['counters']['frames'] == 0 and got['pcm'].shape == (0, 2)
    # a stream that has ended takes no more; a table of the wrong size is refused
    with pytest.raises(native.LDGError, match='ended'):
        ctx.efmdec_feed(rl)
    with pytest.raises(native.LDGError):
        ctx.efmdec_set_table(np.zeros(100, dtype=np.uint16))


def run(args, **kw):
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=600, **kw)


def test_efm_decode_tool(tmp_path):
    ref = R.reference('burst24')
    src, out = str(tmp_path / 'in.efm'), str(tmp_path / 'o')
    R.stream('burst24').tofile(src)
    r = run([TOOL, '--chunk-bytes', '4096', '--stats', src, out])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert open(out + '.efm.pcm', 'rb').read() == ref['pcm'].astype('<i2').tobytes()
    s = json.load(open(out + '.efm.pcm.json'))
    for k in efmdec.COUNTERS:
        assert s[k] == ref['counters'][k], k
    q = R.q_decode(ref['subcode'])
    assert s['q'] == {'sections': q['sections'], 'crc_good': q['crc_good'], 'first_time': list(q['first_time']),
                      'last_time': list(q['last_time'])}
    assert s['q']['crc_good'] == 3 and s['flagged_samples'] == int(ref['flags'].any(axis=1).sum())
    assert any(k.startswith('efmdec_c2') for k in s['kernels_ms'])
    # another table file is honoured; a broken one is refused before the device is touched
    alt = str(tmp_path / 'table.txt')
    with open(efmdec.DEFAULT_TABLE) as fh:
        lines = fh.read().split()
    open(alt, 'w').write('\n'.join(lines) + '\n')
    r = run([TOOL, '--efm-table', alt, src, out + 'b'])
    assert r.returncode == 0 and open(out + 'b.efm.pcm', 'rb').read() == open(out + '.efm.pcm', 'rb').read()
    open(alt, 'w').write('\n'.join(lines[:255]) + '\n')
    r = run([TOOL, '--efm-table', alt, src, out + 'c'])
    assert r.returncode == 1 and 'ERROR' in r.stdout and not os.path.exists(out + 'c.efm.pcm')


def rf_frames(n_samples):
    return int(n_samples / (588 * E.FS / E.FC)) + 2


def test_rf_to_pcm():
    """A 2.5-segment u8 capture of the encoder's frames (amp 12 LSB under the FM carrier, sigma
    2, clock 1) through ldg_efm_extract and the decode: the samples equal the source.  The
    capture's first frame is lost to the filter's reach, so the decoded stream is aligned by the
    Q time code of its first section."""
    nf = rf_frames(E.N_FIX)
    pcm = R.source(nf, seed=9)
    rl, _, _ = R.encode(pcm, nf)
    w, _ = E.efm_wave(rl.astype(np.int64), E.N_FIX, 300.25, 1.0)
    raw = E.pack(E.MID['u8'] + E.fm_carrier(E.N_FIX) + 12.0 * w + np.random.default_rng(77).normal(0, 2.0, E.N_FIX), 'u8')
    ctx = context()
    ctx.efm_set_opts(efm.taps())
    by, _ = ctx.efm_extract(raw, 0, 0, E.N_FIX, 0, E.n_segments(E.N_FIX))
    got = efmdec.decode(ctx, by)
    k = got['counters']
    print(k)
    assert k['frames'] >= nf - 8 and k['samples'] == 6 * (k['frames'] - 111)
    q = efmdec.q_decode(got['subcode'])
    assert q['sections'] >= 3 and q['crc_good'] == q['sections']
    a = int(np.nonzero((got['subcode'][:-1] == efmdec.SYM_S0) & (got['subcode'][1:] == efmdec.SYM_S1))[0][0])
    m, s, f = q['first_time']
    lead = 98 * (75 * (60 * m + s) + f) - a            # source frames before the first decoded one
    assert 0 <= lead <= 8
    assert np.array_equal(got['pcm'], pcm[6 * lead:6 * lead + k['samples']]) and not got['flags'].any()


def test_lddecode_efm_pcm_switch(tmp_path):
    from ldgpu.synth import make_capture
    x = np.frombuffer(make_capture(int(40e6 * 0.2), 'u8'), dtype=np.uint8).astype(np.float64)
    nf = rf_frames(x.size)
    rl, _, _ = R.encode(R.source(nf, seed=31), nf)
    w, _ = E.efm_wave(rl.astype(np.int64), x.size, 300.25, 1.0)
    path = str(tmp_path / 'disc.u8')
    with open(path, 'wb') as fh:
        fh.write(E.pack(x + 12.0 * w, 'u8'))
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'dig')
    r0 = run([DECODE, '-l', '2', path, a])
    r1 = run([DECODE, '-l', '2', '--efm-pcm', path, b])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr[-2000:] + r1.stdout[-2000:] + r1.stderr[-2000:]
    for ext in ('.tbc', '.pcm', '.json'):
        assert open(a + ext, 'rb').read() == open(b + ext, 'rb').read(), ext
    assert not os.path.exists(a + '.efm') and not os.path.exists(a + '.efm.pcm')
    for ext in ('.efm', '.efm.json', '.efm.pcm', '.efm.pcm.json'):
        assert os.path.exists(b + ext), ext
    # the decode of the .efm it wrote, as the library gives it in one call
    got = efmdec.decode(context(), np.fromfile(b + '.efm', dtype=np.uint8))
    assert open(b + '.efm.pcm', 'rb').read() == got['pcm'].astype('<i2').tobytes()
    s = json.load(open(b + '.efm.pcm.json'))
    assert s['frames'] == got['counters']['frames'] > 200 and s['samples'] == got['pcm'].shape[0] > 0
    assert s['q'] == efmdec.q_decode(got['subcode']) and s['flagged'] == got['counters']['flagged']
    # the same refusals as --efm
    r = run([DECODE, '-l', '2', '--efm-pcm', '--epoch-frames', '2', path, str(tmp_path / 'x')])
    assert r.returncode == 1 and '--efm' in r.stdout and not os.path.exists(str(tmp_path / 'x.tbc'))
