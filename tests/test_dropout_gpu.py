"""RF dropout detection and concealment on the GPU (csrc/dropout.hip) against the numpy
restatement of the build-defined rule (tests/dropout_ref.py), on the
shared capture with synthesised dropouts: ldg_field_dropouts exactly equal to the
restatement on the GPU's own arrays and within a pixel of it on the oracle's, the concealed
frames exactly the restatement's copies, and the CLI's --dropouts / --conceal outputs, one
process and sharded."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import dropout_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
SYSTEMS = ['NTSC', 'PAL']
_cache = {}


def field_runs(system):
    """Every field read of the oracle's chain decoded into its own slot of a bare context;
    per field (record, ldg_field_dropouts' runs, the restatement on the GPU's own arrays:
    ldg_debug_read 0 and 24 and the record's linecount)."""
    if ('runs', system) in _cache:
        return _cache['runs', system]
    from ldgpu import native
    from ldgpu.rfparams import RFTables
    dec = R.oracle_decode(system)
    mtf = {x['readsample']: x['mtf_level'] for m in dec['meta'] for x in m['fields']}
    starts = [f['readsample'] for f in dec['fields']]
    rf = RFTables(system)
    ctx = native.Context(system, 0, max_reads=len(starts))
    try:
        ctx.set_filters(rf.params(), rf.tables)
        buf = np.frombuffer(R.capture(system), np.uint8)
        ctx.set_capture(buf, buf.size, 0, 0)
        infos = ctx.decode_reads(starts, [mtf[s] for s in starts])
        slots = list(range(len(starts)))
        out = np.zeros((len(starts), 64, 4), dtype=np.int16)
        counts = np.zeros(len(starts), dtype=np.int32)
        sl = np.arange(len(starts), dtype=np.int32)
        off = ctx.lib.ldg_field_dropouts(ctx.h, len(starts), sl.ctypes.data, out.ctypes.data, 64, counts.ctypes.data)
        ctx.set_dropout_opts({})
        got = ctx.field_dropouts(slots)
        small = ctx.lib.ldg_field_dropouts(ctx.h, len(starts), sl.ctypes.data, out.ctypes.data, 2, counts.ctypes.data)
        res = []
        for i, info in enumerate(infos):
            own = raw = None
            if info.status == native.FS_VALID:
                dm = ctx.debug(i, 0, np.float64, int(info.n_out))
                ll = ctx.debug(i, 24, np.float64, native.MAX_LINES)
                own = R.detect_field(dm, ll, info.linecount, system)
                raw = (ctx.debug(i, 60, np.int16, native.MAX_LINES * 16).reshape(native.MAX_LINES, 8, 2),
                       ctx.debug(i, 61, np.int32, native.MAX_LINES))
            res.append({'status': info.status, 'linecount': info.linecount, 'got': got[i], 'own': own, 'raw': raw})
        ctx.set_dropout_opts(None)
        off2 = ctx.lib.ldg_field_dropouts(ctx.h, len(starts), sl.ctypes.data, out.ctypes.data, 64, counts.ctypes.data)
    finally:
        ctx.close()
    _cache['runs', system] = {'fields': res, 'rc_off': (off, off2), 'rc_small': small}
    return _cache['runs', system]


def gpu_decode(system, opts):
    """(frames, metas) of the shared capture through GPUDecoder(dropouts=opts)."""
    key = ('dec', system, json.dumps(opts, sort_keys=True))
    if key not in _cache:
        from ldgpu.decoder import GPUDecoder
        dec = GPUDecoder(system=system, batch=16, dropouts=opts)
        try:
            dec.set_capture(R.capture(system), 0)
            out = []
            dec.decode(sink=lambda fr, au, m: out.append((np.array(fr, copy=True), m)))
        finally:
            dec.ctx.close()
        _cache[key] = ([f for f, _ in out], [m for _, m in out])
    return _cache[key]


def frame_fields(meta):
    """The records of a frame's top and bottom fields (readframe keeps the last of each)."""
    valid = [x for x in meta['fields'] if x['valid']]
    return [x for x in valid if x['istop']][-1], [x for x in valid if not x['istop']][-1]


@pytest.mark.parametrize('system', SYSTEMS)
def test_detection_equals_restatement_on_gpu_arrays(system):
    fields = field_runs(system)['fields']
    assert sum(f['own'] is not None for f in fields) >= 9
    total = 0
    for f in fields:
        if f['own'] is None:
            continue
        got = [tuple(int(v) for v in row) for row in f['got']]
        print('%s: %d runs' % (system, len(got)))
        assert got == f['own']
        total += len(got)
        runs, cnt = f['raw']                       # ldg_debug_read 60 / 61: the slot's raw arrays
        rows = [r for r, _, _ in f['own']]
        assert [int(c) for c in cnt[:f['linecount']]] == [rows.count(r) for r in range(f['linecount'])]
        assert [(r, int(runs[r, k, 0]), int(runs[r, k, 1])) for r in range(f['linecount']) for k in range(cnt[r])] == f['own']
    # 15 synthesised dropouts, the longest over four rows (+3), at most one absorbed at the cap
    assert total >= 17
    # the capture's cluster fills a row's eight runs on PAL (seven on NTSC)
    most = max(sum(1 for r, _, _ in f['own'] if r == row) for f in fields if f['own'] for row, _, _ in f['own'])
    assert most == (R.MAX_PER_LINE if system == 'PAL' else 7)


@pytest.mark.parametrize('system', SYSTEMS)
def test_detection_matches_oracle_arrays(system):
    """Same rows and counts as the restatement on the oracle's demod and line locations;
    the line locations agree to 1e-6 samples, so a boundary moves by a floor or ceil at most."""
    fields = field_runs(system)['fields']
    oracle = R.oracle_decode(system)['fields']
    assert len(fields) == len(oracle)
    for f, o in zip(fields, oracle):
        assert (f['status'] == 0) == o['valid']
        if not o['valid']:
            continue
        got = [tuple(int(v) for v in row) for row in f['got']]
        assert [r for r, _, _ in got] == [r for r, _, _ in o['runs']]
        worst = max([0] + [max(abs(a[1] - b[1]), abs(a[2] - b[2])) for a, b in zip(got, o['runs'])])
        print('%s read %d: %d runs, max boundary difference %d px' % (system, o['readsample'], len(got), worst))
        assert worst <= 1


@pytest.mark.parametrize('system', SYSTEMS)
def test_invalid_field_and_unset_state(system):
    from ldgpu import native
    res = field_runs(system)
    assert res['rc_off'] == (-4, -4)               # LDG_ESTATE before the options are set and after NULL
    assert res['rc_small'] == -1                   # LDG_EINVAL: out_stride 2 cannot hold a field's runs
    first = res['fields'][0]
    assert first['status'] != native.FS_VALID and first['got'] is None      # counts[i] == -1


@pytest.mark.parametrize('system', SYSTEMS)
def test_concealed_frames_equal_restatement(system):
    plain, metas0 = gpu_decode(system, None)
    detect, metas1 = gpu_decode(system, {})
    concealed, metas2 = gpu_decode(system, {'conceal': 1})
    oracle = R.oracle_decode(system)
    # off (and detection alone): today's frames and metadata
    assert len(plain) == len(oracle['frames']) == len(detect) == len(concealed)
    assert metas0 == oracle['meta']
    for a, b, o in zip(plain, detect, oracle['frames']):
        assert np.array_equal(a, b)
        assert np.abs(a.astype(np.int64) - o.astype(np.int64)).max() <= 1
    assert all('dropouts' not in x for m in metas0 for x in m['fields'])
    strip = [dict(m, fields=[{k: v for k, v in x.items() if k != 'dropouts'} for x in m['fields']]) for m in metas1]
    assert strip == metas0 and metas1 == metas2
    assert all(('dropouts' in x) == x['valid'] for m in metas1 for x in m['fields'])
    changed = fallback = 0
    d = R.LINE_STEP[system]
    for fr, got, m in zip(plain, concealed, metas2):
        top, bot = frame_fields(m)
        want, log = R.conceal_frame(fr, [tuple(r) for r in top['dropouts']], [tuple(r) for r in bot['dropouts']],
                                    top['linecount'], bot['linecount'], system)
        assert np.array_equal(np.asarray(got).reshape(want.shape), want)
        changed += int((want != np.asarray(fr).reshape(want.shape)).sum())
        fallback += sum(1 for p, r, sx, ex, c in log if c == r + d)
    print('%s: %d pixels concealed, %d runs from r + d' % (system, changed, fallback))
    assert changed > 0 and fallback >= 1


def run_cli(*args, nproc=1):
    cmd = [sys.executable, CLI, *map(str, args)]
    env = dict(os.environ)
    if nproc > 1:
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc),
               '--master-addr', '127.0.0.1', '--master-port', str(port), CLI, *map(str, args)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


@pytest.fixture(scope='module')
def cli_runs(tmp_path_factory):
    """The NTSC capture through the CLI: plain --comb, and --conceal --comb."""
    d = tmp_path_factory.mktemp('dropout_cli')
    cap = d / 'cap.u8'
    cap.write_bytes(bytes(R.capture('NTSC')))
    run_cli('--comb', cap, d / 'plain')
    run_cli('--conceal', '--comb', cap, d / 'conc')
    return d, cap


def test_cli_conceal_comb(cli_runs):
    d, _ = cli_runs
    concealed, metas = gpu_decode('NTSC', {'conceal': 1})
    plain, _ = gpu_decode('NTSC', None)
    tbc = np.fromfile(str(d / 'conc.tbc'), dtype=np.uint16).reshape(-1, 525 * 910)
    assert len(tbc) == len(concealed) and all(np.array_equal(a, b) for a, b in zip(tbc, concealed))
    assert json.load(open(d / 'conc.json')) == metas
    assert (d / 'conc.pcm').read_bytes() == (d / 'plain.pcm').read_bytes()
    rgb0 = np.fromfile(str(d / 'plain.rgb'), dtype=np.uint16).reshape(-1, 480, 744, 3)
    rgb1 = np.fromfile(str(d / 'conc.rgb'), dtype=np.uint16).reshape(-1, 480, 744, 3)
    assert rgb0.shape == rgb1.shape and len(rgb0) == len(tbc)
    differ = 0
    for k in range(len(tbc)):
        # rgb row y is frame line 38 + y, combed with the lines two above and below it
        rows = np.flatnonzero((np.asarray(plain[k]).reshape(525, 910) != tbc[k].reshape(525, 910)).any(axis=1))
        fed = {int(r) + o - 38 for r in rows for o in (-2, 0, 2)}
        got = set(np.flatnonzero((rgb0[k] != rgb1[k]).any(axis=(1, 2))).tolist())
        assert got <= fed, (k, sorted(got - fed))
        differ += len(got)
    assert differ > 0


def test_cli_without_the_flags(cli_runs):
    d, _ = cli_runs
    plain, metas = gpu_decode('NTSC', None)
    meta = json.load(open(d / 'plain.json'))
    assert meta == metas and 'dropouts' not in json.dumps(meta)
    tbc = np.fromfile(str(d / 'plain.tbc'), dtype=np.uint16).reshape(-1, 525 * 910)
    assert len(tbc) == len(plain) and all(np.array_equal(a, b) for a, b in zip(tbc, plain))
    from ldgpu.decoder import GPUDecoder
    dec = GPUDecoder(system='NTSC', batch=16)
    try:
        dec.set_capture(R.capture('NTSC'), 0)
        rgb = []
        dec.decode(sink=lambda fr, au, m: None, comb=True, comb_sink=lambda r: rgb.append(np.array(r, copy=True)))
    finally:
        dec.ctx.close()
    assert np.array_equal(np.fromfile(str(d / 'plain.rgb'), dtype=np.uint16), np.concatenate([r.ravel() for r in rgb]))


def test_cli_rejects_cut_and_accepts_thresholds(cli_runs):
    d, cap = cli_runs
    r = subprocess.run([sys.executable, CLI, '-c', '--dropouts', str(cap), str(d / 'cut')], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 1 and '--dropouts' in r.stdout
    # thresholds no sample leaves: no runs, and --dropouts alone leaves the frames as they are
    run_cli('--dropouts', '--dropout-lo-ire', -1000, '--dropout-hi-ire', 1000, cap, d / 'wide')
    meta = json.load(open(d / 'wide.json'))
    assert all(x['dropouts'] == [] for m in meta for x in m['fields'] if x['valid'])
    assert (d / 'wide.tbc').read_bytes() == (d / 'plain.tbc').read_bytes()


def test_cli_pal_and_comb_3d(cli_runs, tmp_path):
    """-p and --comb-3d take the same concealed frames (the 3D comb runs on host frames
    assembled by ldg_assemble_frames, PAL through the fused Y/C decoder)."""
    d, cap = cli_runs
    concealed, metas = gpu_decode('NTSC', {'conceal': 1})
    run_cli('--conceal', '--comb', '--comb-3d', cap, d / 'c3d')
    tbc = np.fromfile(str(d / 'c3d.tbc'), dtype=np.uint16).reshape(-1, 525 * 910)
    assert len(tbc) == len(concealed) and all(np.array_equal(a, b) for a, b in zip(tbc, concealed))
    assert json.load(open(d / 'c3d.json')) == metas
    assert os.path.getsize(d / 'c3d.rgb') == (len(tbc) - 2) * 480 * 744 * 3 * 2
    pcap = tmp_path / 'pal.u8'
    pcap.write_bytes(bytes(R.capture('PAL')))
    concealed, metas = gpu_decode('PAL', {'conceal': 1})
    run_cli('-p', '--conceal', '--comb', pcap, tmp_path / 'pal')
    tbc = np.fromfile(str(tmp_path / 'pal.tbc'), dtype=np.uint16).reshape(-1, 625 * 1135)
    assert len(tbc) == len(concealed) and all(np.array_equal(a, b) for a, b in zip(tbc, concealed))
    assert json.load(open(tmp_path / 'pal.json')) == metas
    assert os.path.getsize(tmp_path / 'pal.rgb') == len(tbc) * 576 * 1057 * 3 * 2


def test_cli_sharded_equals_single(cli_runs):
    """Two gloo ranks on one device write the single process's files byte for byte:
    detection and concealment are pure functions of one field and its frame."""
    d, cap = cli_runs
    run_cli('--conceal', '--comb', cap, d / 'two', nproc=2)
    for ext in ('.tbc', '.json', '.rgb', '.pcm'):
        assert (d / ('two' + ext)).read_bytes() == (d / ('conc' + ext)).read_bytes(), ext
    # and in epochs of two frames in one process
    run_cli('--conceal', '--comb', '--epoch-frames', 2, cap, d / 'ep')
    for ext in ('.tbc', '.json', '.rgb'):
        assert (d / ('ep' + ext)).read_bytes() == (d / ('conc' + ext)).read_bytes(), ext
