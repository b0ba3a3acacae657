"""EFM run-length extraction on the GPU (csrc/efm.hip) against the numpy restatement of the
build-defined rule (tests/efm_ref.py): z, the crossing times, the
bytes and the per-segment counters for the four capture formats and three clocks; chunking,
host and device windows, the ignored spike pair, empty inputs; efm_extract.py and
lddecode.py --efm end to end.  The fixtures' conditioning (tests/test_efm_ref.py) is what
lets bytes and counters be compared exactly."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import efm_ref as R
from ldgpu import efm, native
from ldgpu.formats import NAME_TO_FMT, samples_in_bytes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DECODE = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
EXTRACT = os.path.join(ROOT, 'ld-decode_amd', 'efm_extract.py')
COUNTERS = ('emitted', 'ignored', 'clamped_low', 'clamped_high')
_ctx = []


def context():
    if not _ctx:
        _ctx.append(native.Context('NTSC', 0, max_reads=1))
    return _ctx[0]


def teardown_module(module):
    for c in _ctx:
        c.close()
    _ctx.clear()


def whole(ctx, raw, fmt, **opts):
    """The whole file in one call: (bytes, per-segment counters)."""
    n = samples_in_bytes(fmt, len(raw))
    ctx.efm_set_opts(efm.taps(), **opts)
    return ctx.efm_extract(raw, fmt, 0, n, 0, R.n_segments(n))


def check_segments(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [g[k] for k in COUNTERS] == [w[k] for k in COUNTERS]
        assert abs(g['final_P'] - w['final_P']) <= 1e-12 * w['final_P'], (g['final_P'], w['final_P'])


@pytest.mark.parametrize('fmt,clk', R.FIXTURES)
def test_parity_with_the_restatement(fmt, clk):
    raw, _, _, ref = R.fixture(fmt, clk)
    ctx = context()
    by, segs = whole(ctx, raw, NAME_TO_FMT[fmt], keep_debug=True)
    first, z = ctx.efm_debug('z')
    times = ctx.efm_debug('times')
    zr = ref['z']
    ok = np.nonzero(np.isfinite(zr))[0]
    assert first == ok[0] and first + z.size == ok[-1] + 1 and np.isfinite(zr[first:first + z.size]).all()
    dz = np.abs(z - zr[first:first + z.size]).max()
    assert times.size == ref['times'].size
    dt = np.abs(times - ref['times']).max()
    print('%s clock %g: max |z - ref| %.3g, %d crossings, max |t - ref| %.3g, %d bytes' % (fmt, clk, dz, times.size, dt, by.size))
    assert dz <= 1e-9
    assert dt <= 1e-7
    assert np.array_equal(by, ref['bytes'])
    check_segments(segs, ref['segments'])


def test_chunking_does_not_change_the_bytes():
    raw, _, _, ref = R.fixture('u8', 1.0)
    ctx = context()
    buf = np.frombuffer(raw, dtype=np.uint8)
    for chunk in (1, 3):
        by, segs = efm.extract(ctx, buf, 0, chunk_segments=chunk)
        assert np.array_equal(by, ref['bytes']), chunk
        check_segments(segs, ref['segments'])
    # a range of its own, from its window alone
    by, segs = efm.extract(ctx, buf, 0, 1, 2)
    a = ref['segments'][0]['emitted']
    assert np.array_equal(by, ref['bytes'][a:a + ref['segments'][1]['emitted']])
    # a window that does not cover the range's halo is refused
    lo, hi = native.efm_window(1, 2, buf.size)
    with pytest.raises(native.LDGError, match='does not cover'):
        ctx.efm_extract(buf[lo + 12:hi], 0, lo + 12, buf.size, 1, 2)


def hip_runtime():
    """The HIP runtime libldgpu.so is linked against, as loaded into this process."""
    native.load()
    with open('/proc/self/maps') as fh:
        path = next(line.split()[-1] for line in fh if 'libamdhip64' in line)
    hip = C.CDLL(path)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize('fmt', ['u8', 'lds'])
def test_device_window_equals_host_window(fmt):
    raw, _, _, ref = R.fixture(fmt, 1.0)
    f = NAME_TO_FMT[fmt]
    ctx = context()
    ctx.efm_set_opts(efm.taps())
    buf = np.frombuffer(raw, dtype=np.uint8)
    n = samples_in_bytes(f, buf.size)
    lo, hi = native.efm_window(1, 3, n)
    b0 = efm.sample_byte(f, lo)
    win = np.ascontiguousarray(buf[b0:])
    host = ctx.efm_extract(win, f, lo, n, 1, 3)
    hip = hip_runtime()
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), win.size) == 0
    try:
        assert hip.hipMemcpy(dev, win.ctypes.data, win.size, 1) == 0          # hipMemcpyHostToDevice
        got = ctx.efm_extract(None, f, lo, n, 1, 3, device_ptr=dev.value, nbytes=win.size)
    finally:
        hip.hipFree(dev)
    assert np.array_equal(got[0], host[0]) and got[1] == host[1]
    a = ref['segments'][0]['emitted']
    assert np.array_equal(host[0], ref['bytes'][a:])
    check_segments(host[1], ref['segments'][1:])


def test_spike_pair_is_ignored():
    raw, ref = R.spike_fixture()
    by, segs = whole(context(), raw, 0)
    assert [s['ignored'] for s in ref['segments']] == [0, 1, 0]
    assert np.array_equal(by, ref['bytes'])
    check_segments(segs, ref['segments'])


def test_empty_inputs():
    ctx = context()
    p0 = R.FS / R.FC
    by, segs = whole(ctx, np.full(3 * R.L // 2, 128, dtype=np.uint8).tobytes(), 0)
    assert by.size == 0 and [s['emitted'] for s in segs] == [0, 0] and all(s['final_P'] == p0 for s in segs)
    for n in (0, 100, 2683):
        by, segs = whole(ctx, (np.arange(n) % 251).astype(np.uint8).tobytes(), 0)
        assert by.size == 0 and all(s['emitted'] == 0 and s['final_P'] == p0 for s in segs)
    with pytest.raises(native.LDGError):
        ctx.efm_set_opts(efm.taps()[:-1])


# ---- the tools ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def disc(tmp_path_factory):
    """0.3 s of synthetic NTSC RF with EFM added: (path, restatement of the whole file)."""
    from ldgpu.synth import make_capture
    raw, _, _ = R.add_efm(make_capture(int(40e6 * 0.3), 'u8'), seed=21)
    path = str(tmp_path_factory.mktemp('efm') / 'disc.u8')
    with open(path, 'wb') as fh:
        fh.write(raw)
    return path, R.extract(R.samples(raw, 0))


def run(args, **kw):
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=600, **kw)


def test_efm_extract_tool(disc, tmp_path):
    path, ref = disc
    out = str(tmp_path / 'o')
    r = run([EXTRACT, '--chunk-segments', '5', '--stats', path, out])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    by = np.fromfile(out + '.efm', dtype=np.uint8)
    assert ref['min_dz'] > 1e-6 and ref['min_round'] > 1e-6
    assert np.array_equal(by, ref['bytes'])
    s = json.load(open(out + '.efm.json'))
    want = efm.summarise(ref['bytes'], ref['segments'])
    for k in ('segments', 'run_lengths', 'histogram', 'ignored', 'clamped_low', 'clamped_high', 'syncs', 'frames_588'):
        assert s[k] == want[k], k
    assert s['frames_588'] > 0.9 * s['syncs'] > 100
    assert abs(s['final_period_ratio']['mean'] - 1) < 1e-3
    assert any(k.startswith('efm_fir') for k in s['kernels_ms'])
    # a sample range is widened outward to whole segments
    r = run([EXTRACT, '--start-sample', str(3 * R.L + 5), '--end-sample', str(5 * R.L - 7), path, out + 'r'])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    e = [g['emitted'] for g in ref['segments']]
    assert np.array_equal(np.fromfile(out + 'r.efm', dtype=np.uint8), ref['bytes'][sum(e[:3]):sum(e[:5])])
    assert json.load(open(out + 'r.efm.json'))['samples'] == [3 * R.L, 5 * R.L]


def test_lddecode_efm_switch(disc, tmp_path):
    path, ref = disc
    a, b = str(tmp_path / 'plain'), str(tmp_path / 'efm')
    r0 = run([DECODE, '-l', '4', path, a])
    r1 = run([DECODE, '-l', '4', '--efm', path, b])
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr[-2000:] + r1.stdout[-2000:] + r1.stderr[-2000:]
    for ext in ('.tbc', '.pcm', '.json'):
        assert open(a + ext, 'rb').read() == open(b + ext, 'rb').read(), ext
    assert not os.path.exists(a + '.efm')
    meta = json.load(open(b + '.json'))
    first, last = meta[0]['fields'][0]['readsample'], meta[-1]['nextsample']
    lo, hi = efm.segment_range(first, last, os.path.getsize(path))
    e = [g['emitted'] for g in ref['segments']]
    assert hi > lo
    assert np.array_equal(np.fromfile(b + '.efm', dtype=np.uint8), ref['bytes'][sum(e[:lo]):sum(e[:hi])])
    s = json.load(open(b + '.efm.json'))
    assert s['first_segment'] == lo and s['segments'] == hi - lo
    # the same bytes as the tool over that range
    r = run([EXTRACT, '--start-sample', str(first), '--end-sample', str(last), path, a])
    assert r.returncode == 0 and open(a + '.efm', 'rb').read() == open(b + '.efm', 'rb').read()
    # refused where the decode is not one plain pass
    r = run([DECODE, '-l', '4', '--efm', '--epoch-frames', '2', path, str(tmp_path / 'x')])
    assert r.returncode == 1 and '--efm' in r.stdout and not os.path.exists(str(tmp_path / 'x.tbc'))
