"""The NTSC line services on the GPU (csrc/lines.hip) against the numpy restatement of the
build-defined rule (tests/lines_ref.py): ldg_frames_line_services and
ldg_field_line_services exactly equal to the restatement, on ideal rows, random rows and the rows
of the table's captures as the GPU itself decoded them (where they must also say what the table
says); the whole decode of a capture that carries a known sequence; and the command-line tools,
one process and sharded."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import lines_ref as R

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, 'ld-decode_amd', 'lddecode.py')
TOOL = os.path.join(ROOT, 'ld-decode_amd', 'process_vbi.py')
_cache = {}


# ---- layout (no GPU needed) ---------------------------------------------------------------------
def test_line_services_layout_matches_header(tmp_path):
    """The ctypes mirror of ldg_line_services == the C compiler's view of include/ldgpu.h."""
    from ldgpu import native
    members = [k for k, _ in native.LineServices._fields_]
    src = tmp_path / 'ls.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ldgpu.h"\nint main(void){'
                   'printf("%zu %d", sizeof(ldg_line_services), LDG_LINE_SERVICES_SIZE);' +
                   ''.join('printf(" %%zu", offsetof(ldg_line_services, %s));' % k for k in members) +
                   'printf(" %d %d %d %d\\n", LDG_LINE_ABSENT, LDG_LINE_OK, LDG_LINE_CHECK, LDG_LINE_FRAME);return 0;}')
    exe = tmp_path / 'ls'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    L = native.LineServices
    assert got == [C.sizeof(L), native.LINE_SERVICES_SIZE] + [getattr(L, k).offset for k in members] + \
        [native.LINE_ABSENT, native.LINE_OK, native.LINE_CHECK, native.LINE_FRAME]
    assert np.dtype(L).itemsize == 36 and (R.ABSENT, R.OK, R.CHECK, R.FRAME) == (0, 1, 2, 3)
    assert {'ldg_field_line_services', 'ldg_frames_line_services'} <= set(native.EXPORTS)


# ---- kernel against restatement -----------------------------------------------------------------
def known_fields():
    """Fields of ideal rows at the edges of the rule's comparisons (test_lines_ref.py asserts their
    answers), then seeded random ones: 66 in all."""
    T25, T35, T50 = R.T25, R.T35, R.T50
    F = []
    for xs in (269, 270, 409, 410):
        F.append(R.ideal_field(cc=R.ideal_cc(xs, 0xFF, 0xFF), vid=R.ideal_vid(xs - 210, R.vid_word(0x3FFF))))
    for rises in (5, 6, 8, 9):
        F.append(R.ideal_field(cc=R.ideal_cc(339, 0xC1, 0x79, rises=rises), white=R.ideal_white(335 + rises)))
    p = R.ideal_cc(339, 0xFF, 0xFF, rises=6)
    v = R.ideal_vid(100, R.vid_word(0))
    v[40:80] = T35 + 1
    for d, t in ((41, T25 + 1), (40, T25 + 1), (40, T25)):
        q, w = p.copy(), v.copy()
        q[339 - d] = t
        w[80] = t - T25 + T35 if d == 40 else R.L0
        F.append(R.ideal_field(cc=q, vid=w))
    p = R.ideal_cc(339, 0xC1, 0x79)
    c = R.cc_centre(339, 1)
    v = R.ideal_vid(100, R.vid_word(0x152E))
    for extra in (0, 1):
        q, w = p.copy(), v.copy()
        q[c - 4:c + 5] = T25
        q[c + 4] += extra
        w[784:793] = T35
        w[784] += extra
        F.append(R.ideal_field(cc=q, vid=w, white=R.ideal_white(680, hi=T50 + extra)))
    word = R.vid_word(0x152E)
    for k in (0, 5, 6, 19):
        F.append(R.ideal_field(vid=R.ideal_vid(100, word ^ (1 << k)), cc=R.ideal_cc(300 + k, 0x41, 0xF9)))
    F.append(R.ideal_field(vid=R.ideal_vid(100, word, ref=(1, 1))))
    F.append(R.ideal_field(vid=R.ideal_vid(100, R.vid_word(0x3FFF), ref=(0, 1))))
    p = R.ideal_cc(270, 0xC1, 0x79)
    p[2], p[3] = R.L0, R.L50
    F.append(R.ideal_field(cc=p))
    p = p.copy()
    p[2] = R.L50
    F.append(R.ideal_field(cc=p))
    for value in (0, 65535):
        F.append(np.full((R.ROWS, R.W), value, dtype=np.uint16))
    for count in (0, 340, 341, 680):
        F.append(R.ideal_field(white=R.ideal_white(count)))
    rng = np.random.default_rng(20240612)
    levels = np.array([0, R.L0, T25 - 1, T25, T25 + 1, T35 - 1, T35, T35 + 1, T50 - 1, T50, T50 + 1, R.L100, 65535])
    while len(F) < 66:
        kind = len(F) % 3
        if kind == 0:                                  # uniform random pixels
            rows = rng.integers(0, 65536, (R.ROWS, R.W)).astype(np.uint16)
        elif kind == 1:                                # random segments of levels next to the thresholds
            rows = np.zeros((R.ROWS, R.W), dtype=np.uint16)
            for r in range(R.ROWS):
                x = 0
                while x < R.W:
                    n = int(rng.integers(1, 70))
                    rows[r, x:x + n] = levels[rng.integers(0, len(levels))]
                    x += n
        else:                                          # trains at random places under noise
            rows = R.ideal_field(white=R.ideal_white(int(rng.integers(300, 400))),
                                 cc=R.ideal_cc(int(rng.integers(262, 418)), int(rng.integers(0, 256)),
                                               int(rng.integers(0, 256)), rises=int(rng.integers(4, 11))),
                                 vid=R.ideal_vid(int(rng.integers(52, 168)), int(rng.integers(0, 1 << 20))))
            rows = np.clip(rows.astype(np.int64) + rng.integers(-9000, 9001, rows.shape), 0, 65535).astype(np.uint16)
        F.append(rows)
    return F


def known_frames():
    if 'known' not in _cache:
        F = known_fields()
        assert len(F) == 66
        # fields 2 f and 2 f + 1 make frame f; the rows past 20 and the unused rows are random
        fr = np.random.default_rng(7).integers(0, 65536, (33, 525, R.W)).astype(np.uint16)
        for f in range(33):
            fr[f, 0:2 * R.ROWS:2] = F[2 * f]
            fr[f, 1:2 * R.ROWS:2] = F[2 * f + 1]
        want = R.decode_frames(fr)
        _cache['known'] = (fr, want)
    return _cache['known']


def hip_runtime():
    """hipMalloc / hipMemcpy / hipFree of the HIP runtime libldgpu.so is linked against, resolved
    through the library's own handle (a process may hold a second copy of the runtime)."""
    from ldgpu import native
    hip = native.load()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


@gpu
@pytest.mark.parametrize('n', [1, 2, 33])
def test_frames_form_equals_restatement(n, gpu_ctx_ntsc):
    ctx, _ = gpu_ctx_ntsc
    fr, want = known_frames()
    states = {(a['cc_state'], a['vid_state'], a['white_flag']) for pair in want for a in pair}
    assert {s[0] for s in states} == {s[1] for s in states} == {0, 1, 2, 3} and {s[2] for s in states} == {0, 1}
    assert ctx.frames_line_services(fr[:n]) == want[:n]
    # the other parity: the frames' rows shifted down by one (row 0 random)
    sw = np.roll(fr[:n], 1, axis=1)
    got = ctx.frames_line_services(sw)
    assert [pair[1] for pair in got] == [pair[0] for pair in want[:n]]
    assert got == R.decode_frames(sw)
    # from device memory
    hip = hip_runtime()
    dev = C.c_void_p()
    a = np.ascontiguousarray(fr[:n])
    assert hip.hipMalloc(C.byref(dev), a.nbytes) == 0
    try:
        assert hip.hipMemcpy(dev, a.ctypes.data, a.nbytes, 1) == 0          # hipMemcpyHostToDevice
        assert ctx.frames_line_services(device_ptr=dev.value, n=n) == want[:n]
    finally:
        hip.hipFree(dev)


@gpu
def test_profile_names_the_kernel(gpu_ctx_ntsc):
    ctx, _ = gpu_ctx_ntsc
    fr, _ = known_frames()
    ctx.profile(True)
    try:
        ctx.frames_line_services(fr[:2])
        stats = ctx.profile_stats()
    finally:
        ctx.profile(False)
    assert stats['line_services'][0] == 1


# ---- the slot form on the table's captures ------------------------------------------------------
@gpu
@pytest.mark.parametrize('case', list(R.CASES))
def test_slot_form_on_table(case, gpu_ctx_ntsc):
    """One decode of the case's read: ldg_field_line_services equals the restatement on the rows
    read back from that slot, exactly, and says what the table says."""
    from ldgpu import native
    ctx, _ = gpu_ctx_ntsc
    c = R.CASES[case]
    data = R.capture(case)
    ctx.set_capture(data, data.size, 0, 0)
    info = ctx.decode_reads(c['reads'], [1.0])[0]
    assert info.status == native.FS_VALID
    rec = ctx.field_line_services([0])[0]
    rows = ctx.debug(0, 40, np.uint16, info.linecount * R.W).reshape(info.linecount, R.W)
    print(case, rec)
    assert rec == R.decode_field(rows)
    assert R.matches(rec, c['expect'][0]) == []


@gpu
def test_invalid_slot_and_order(gpu_ctx_ntsc):
    """A field that is not valid gives white_count -1 and every state absent; records come back in
    the order of `slots`."""
    from ldgpu import native
    ctx, _ = gpu_ctx_ntsc
    data = R.capture('clean')
    ctx.set_capture(data, data.size, 0, 0)
    infos = ctx.decode_reads([0, R.START['NTSC']], [1.0, 1.0], slots=[5, 2])
    assert infos[0].status != native.FS_VALID and infos[1].status == native.FS_VALID
    a, b = ctx.field_line_services([5, 2])
    assert a == R.NO_FIELD
    assert R.matches(b, R.CASES['clean']['expect'][0]) == []
    assert ctx.field_line_services([2, 5]) == [b, a]


# ---- argument checks ----------------------------------------------------------------------------
@gpu
def test_argument_checks(gpu_ctx_ntsc, gpu_ctx_pal):
    from ldgpu import native
    ctx, _ = gpu_ctx_ntsc
    pal, _ = gpu_ctx_pal
    lib = ctx.lib
    out = np.zeros((2, 2), dtype=np.dtype(native.LineServices))
    sl = np.zeros(2, dtype=np.int32)
    fr = np.zeros((1, 525 * 910), dtype=np.uint16)
    err = lambda c: lib.ldg_last_error(c.h).decode()     # noqa: E731
    # PAL: both refused, also for n == 0
    for n in (0, 1):
        assert lib.ldg_field_line_services(pal.h, n, sl.ctypes.data, out.ctypes.data) == -1 and 'PAL' in err(pal)
        assert lib.ldg_frames_line_services(pal.h, n, fr.ctypes.data, 0, out.ctypes.data) == -1 and 'PAL' in err(pal)
    # n == 0 does nothing (no pointer is read); n < 0 and NULL pointers are named
    assert lib.ldg_field_line_services(ctx.h, 0, None, None) == 0
    assert lib.ldg_frames_line_services(ctx.h, 0, None, 0, None) == 0
    assert lib.ldg_field_line_services(ctx.h, -1, sl.ctypes.data, out.ctypes.data) == -1 and 'n must' in err(ctx)
    assert lib.ldg_frames_line_services(ctx.h, -1, fr.ctypes.data, 0, out.ctypes.data) == -1 and 'n must' in err(ctx)
    assert lib.ldg_field_line_services(ctx.h, 1, None, out.ctypes.data) == -1 and 'slots' in err(ctx)
    assert lib.ldg_field_line_services(ctx.h, 1, sl.ctypes.data, None) == -1 and 'out' in err(ctx)
    assert lib.ldg_frames_line_services(ctx.h, 1, None, 0, out.ctypes.data) == -1 and 'frames' in err(ctx)
    assert lib.ldg_frames_line_services(ctx.h, 1, None, 1, out.ctypes.data) == -1 and 'frames' in err(ctx)
    assert lib.ldg_frames_line_services(ctx.h, 1, fr.ctypes.data, 0, None) == -1 and 'out' in err(ctx)
    # a slot outside the context, and more slots than it has
    sl[0] = ctx.max_reads
    assert lib.ldg_field_line_services(ctx.h, 1, sl.ctypes.data, out.ctypes.data) == -1 and 'slots' in err(ctx)
    many = np.zeros(ctx.max_reads + 1, dtype=np.int32)
    big = np.zeros(ctx.max_reads + 1, dtype=np.dtype(native.LineServices))
    assert lib.ldg_field_line_services(ctx.h, many.size, many.ctypes.data, big.ctypes.data) == -1 and 'max_reads' in err(ctx)
    assert lib.ldg_field_line_services(None, 1, sl.ctypes.data, out.ctypes.data) == -1
    assert lib.ldg_frames_line_services(None, 1, fr.ctypes.data, 0, out.ctypes.data) == -1


# ---- the whole decode ---------------------------------------------------------------------------
def gpu_decode(batch, on):
    key = ('dec', batch, on)
    if key not in _cache:
        from ldgpu.decoder import GPUDecoder
        dec = GPUDecoder(system='NTSC', batch=batch, line_services=on)
        try:
            dec.set_capture(R.build_whole(), 0)
            out = []
            dec.decode(sink=lambda fr, au, m: out.append((np.array(fr, copy=True), np.array(au, copy=True), m)))
        finally:
            dec.ctx.close()
        _cache[key] = out
    return _cache[key]


def field_sequence(meta):
    """(capture frame, field) of every valid field record of a frame's metadata: the last two are
    the frame's own (its VBI frame number - 200), the ones before them count back from there."""
    k = meta['vbi']['framenr'] - R.BASE['first_frame']
    valid = [x for x in meta['fields'] if x['valid']]
    # record i lies j = len - 1 - i fields before the frame's bottom field
    back = [len(valid) - 1 - i for i in range(len(valid))]
    return list(zip(valid, [(k - j // 2, 1 - j % 2) for j in back]))


@gpu
@pytest.mark.parametrize('batch', [3, 16])
def test_whole_decode_carries_the_sequence(batch):
    on, off = gpu_decode(batch, True), gpu_decode(batch, False)
    assert len(on) == len(off) >= 6
    seen = 0
    for (fr, au, m), (fr0, au0, m0) in zip(on, off):
        assert np.array_equal(fr, fr0) and np.array_equal(au, au0)
        strip = dict(m, fields=[{k: v for k, v in x.items() if k != 'lineServices'} for x in m['fields']])
        assert strip == m0 and 'lineServices' not in json.dumps(m0)
        assert all(('lineServices' in x) == x['valid'] for x in m['fields'])
        for x, (k, fld) in field_sequence(m):
            assert x['istop'] == (fld == 0)
            got, want = x['lineServices'], R.whole_expect(k, fld)
            assert {key: got[key] for key in want} == want, (k, fld, got)
            assert got['whiteCount'] in (0, 680)
            seen += 1
    whites = [x['lineServices']['white'] for _, _, m in on for x in m['fields'] if x['valid']]
    ids = {x['lineServices']['videoId'] for _, _, m in on for x in m['fields'] if x['valid']}
    assert seen >= 13 and True in whites and False in whites and ids == {0x152E, 0x2A51}
    # the frames' own rows through the frames form give the same records
    from ldgpu import native
    ctx = native.Context('NTSC', 0, max_reads=1, max_frames=1)
    try:
        recs = ctx.frames_line_services(np.stack([fr for fr, _, _ in on]))
    finally:
        ctx.close()
    for (fr, au, m), pair in zip(on, recs):
        valid = [x for x in m['fields'] if x['valid']]
        assert [valid[-2]['lineServices'], valid[-1]['lineServices']] == [R.json_record(r) for r in pair]


# ---- the command-line tools ---------------------------------------------------------------------
def run_cli(*args, nproc=1, tool=CLI):
    cmd = [sys.executable, tool, *map(str, args)]
    env = dict(os.environ)
    if nproc > 1:
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc),
               '--master-addr', '127.0.0.1', '--master-port', str(port), tool, *map(str, args)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


@pytest.fixture(scope='module')
def cli_runs(tmp_path_factory):
    """The whole capture through lddecode.py with and without --line-services."""
    d = tmp_path_factory.mktemp('lines_cli')
    cap = d / 'cap.u8'
    cap.write_bytes(R.build_whole())
    run_cli('--line-services', cap, d / 'ls')
    run_cli(cap, d / 'plain')
    return d, cap


@gpu
def test_cli_writes_the_records(cli_runs):
    d, _ = cli_runs
    on, off = gpu_decode(16, True), gpu_decode(16, False)
    assert json.load(open(d / 'ls.json')) == json.loads(json.dumps([m for _, _, m in on]))
    plain = (d / 'plain.json').read_text()
    assert 'lineServices' not in plain and json.loads(plain) == json.loads(json.dumps([m for _, _, m in off]))
    for ext in ('.tbc', '.pcm'):
        assert (d / ('ls' + ext)).read_bytes() == (d / ('plain' + ext)).read_bytes(), ext
    tbc = np.fromfile(str(d / 'plain.tbc'), dtype=np.uint16).reshape(-1, 525 * 910)
    assert len(tbc) == len(off) and all(np.array_equal(a, np.asarray(b).ravel()) for a, (b, _, _) in zip(tbc, off))


@gpu
def test_cli_refuses_pal_and_cut(cli_runs):
    d, cap = cli_runs
    for flag in ('-p', '-c'):
        r = subprocess.run([sys.executable, CLI, flag, '--line-services', str(cap), str(d / 'no')], capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 1 and '--line-services' in r.stdout
        assert not os.path.exists(d / 'no.tbc') and not os.path.exists(d / 'no.r16')


@gpu
def test_process_vbi_equals_the_decode(cli_runs):
    d, _ = cli_runs
    r = run_cli(d / 'ls.tbc', '--stats', tool=TOOL)
    meta = json.load(open(d / 'ls.json'))
    res = json.load(open(d / 'ls.lines.json'))
    assert len(res['frames']) == len(meta)
    flat = []
    for i, (m, f) in enumerate(zip(meta, res['frames'])):
        valid = [x for x in m['fields'] if x['valid']]
        assert f['frame'] == i and f['fields'] == [valid[-2]['lineServices'], valid[-1]['lineServices']]
        flat += f['fields']
    counts = res['counts']
    assert counts['fields'] == 2 * len(meta) and counts['white'] == sum(x['white'] for x in flat) > 0
    assert counts['cc'] == {'absent': 0, 'ok': len(flat), 'check': 0, 'frame': 0} == counts['videoId']
    assert json.loads(r.stdout.strip().splitlines()[-1]) == dict(counts, frames=len(meta))
    # -o names the output
    run_cli(d / 'ls.tbc', '-o', d / 'other', tool=TOOL)
    assert json.load(open(d / 'other.lines.json')) == res


@gpu
def test_cli_sharded_equals_single(cli_runs):
    """Two gloo ranks on one device write the single process's files byte for byte: the records
    are a pure function of one field and travel with it."""
    d, cap = cli_runs
    run_cli('--line-services', cap, d / 'two', nproc=2)
    for ext in ('.tbc', '.json', '.pcm'):
        assert (d / ('two' + ext)).read_bytes() == (d / ('ls' + ext)).read_bytes(), ext


@gpu
def test_cli_epochs_and_manifest(cli_runs):
    """Epochs of two frames write the same .json; a manifest written without the flag does not
    resume with it."""
    d, cap = cli_runs
    run_cli('--line-services', '--epoch-frames', 2, '--manifest', d / 'ep.man', cap, d / 'ep')
    for ext in ('.tbc', '.json'):
        assert (d / ('ep' + ext)).read_bytes() == (d / ('ls' + ext)).read_bytes(), ext
    assert json.load(open(d / 'ep.man'))['line_services'] is True
    run_cli('-l', 2, '--epoch-frames', 2, '--manifest', d / 'off.man', cap, d / 'off')
    assert 'line_services' not in json.load(open(d / 'off.man'))
    r = subprocess.run([sys.executable, CLI, '--line-services', '-l', '2', '--epoch-frames', '2', '--manifest',
                        str(d / 'off.man'), str(cap), str(d / 'off')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and 'belongs to another decode' in r.stdout
