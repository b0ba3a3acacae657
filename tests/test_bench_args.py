"""bench.py's argument checks (CPU, no device): the streamed / host-buffer modes belong to
the NTSC capture workload only, and are refused before anything touches a GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('extra', [['--system', 'PAL', '--stream-file', '/tmp/x'], ['--sharded', '--host-io'],
                                   ['--sharded', '--stream-file', '/tmp/x']])
def test_bench_refuses_io_modes_outside_the_capture_workload(extra):
    env = dict(os.environ, WORLD_SIZE='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *extra], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 2
    assert 'the NTSC capture workload' in r.stderr


def test_bench_refuses_a_run_without_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True,
                       text=True, timeout=120, env=dict(os.environ, WORLD_SIZE='1'))
    assert r.returncode == 2 and '--steps at least 1' in r.stderr


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ldg_bench_args', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_last_frames_walks_the_read_chain_back_from_the_final_position():
    """--dump-outputs picks the last frames of a decode from its read cache: fields chained by
    start + nextfieldoffset back from the final position, paired top / bottom; reads off the
    chain (speculative, invalid) are not taken, and of two reads that end at the same sample
    the one at the lower MTF level is."""
    from types import SimpleNamespace as NS
    from ldgpu import native
    b = _bench()

    def info(nfo, istop, status=native.FS_VALID):
        return NS(status=status, nextfieldoffset=nfo, istop=istop, linecount=263 - istop)
    # fields of 1000 samples from 5000 on: bottom, top, bottom, top, bottom, top (first field bottom)
    cache = {(5000 + 1000 * k, 0.5): (10 + k, info(1000, k % 2)) for k in range(6)}
    cache[(11000, 0.5)] = (30, info(1000, 0))                      # speculative, past the end
    cache[(10500, 0.5)] = (31, info(500, 1, native.FS_SHORT))      # not a valid field
    cache[(10000, 0.25)] = (32, info(1000, 1))                     # the last top field again, lower MTF
    dec = NS(cache=cache, last_meta={'nextsample': 11000})
    # frames pair consecutive fields from the end: (9000, 10000) then (7000, 8000)
    assert b.last_frames(dec, 2) == [(13, 12, 8000, 7000, 262, 263), (32, 14, 10000, 9000, 262, 263)]
    assert b.last_frames(dec, 8)[0][2:4] == (6000, 5000) and len(b.last_frames(dec, 8)) == 3
    assert b.last_frames(NS(cache=cache, last_meta=None), 2) == []
    assert b.last_frames(NS(cache=cache, last_meta={'nextsample': 999}), 2) == []


def _plain_run(out, steps):
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps),
                        '--warmup', '1', '--seconds', '1', '--dump-outputs', str(out)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, WORLD_SIZE='1'))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines                       # the result line is the only stdout output
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_times_its_steps_and_dumps_what_they_decoded(tmp_path):
    """The benchmark's command line (1 s of RF per step): --steps sets the number of timed
    steps, ms_per_step is the timed region over them, a plain run carries none of --full's
    legs, and --dump-outputs writes the last step's outputs, float32 / float64 and under
    64 MB, the same from run to run whatever the number of steps."""
    import numpy as np
    d = _plain_run(tmp_path / 'a', 3)
    assert d['steps'] == 3 and d['warmup'] == 1 and len(d['checks']['step_ms']) == 3
    assert d['unit'] == 'RF Msamples/s' and d['higher_is_better'] is True and d['dtype'] == 'f64'
    # each step ends synchronised, so the region holds the steps' own times and the loop's
    # bookkeeping (step_ms is rounded to 0.01 ms)
    assert abs(d['ms_per_step'] - sum(d['checks']['step_ms']) / 3) < 1.0
    assert d['value'] > 0 and d['checks']['framenr_consecutive']
    assert d['full'] is False and d['roofline'] is None and d['cpu_baseline'] is None and d['kernels_ms'] == {}
    a = {f[:-4]: np.load(tmp_path / 'a' / f) for f in sorted(os.listdir(tmp_path / 'a'))}
    assert set(a) == {'summary', 'frame_numbers', 'frame_starts', 'tbc_frames', 'field_linelocs', 'comb_burst_ema',
                      'comb_state', 'rgb48_frames'}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    nfr = d['config']['frames_per_step']
    assert a['summary'][0] == nfr == a['frame_numbers'].size and nfr > 8
    assert np.array_equal(np.diff(a['frame_numbers']), np.ones(nfr - 1))
    assert a['tbc_frames'].shape == (4, 525 * 910) and a['rgb48_frames'].shape == (4, 480, 744, 3)
    for k in ('tbc_frames', 'rgb48_frames'):             # uint16 pictures with content
        assert np.array_equal(a[k], np.round(a[k])) and a[k].min() >= 0 and a[k].max() <= 65535 and a[k].std() > 1000
    # the frames are the step's last: consecutive fields, the last one ending at the final position
    st = a['frame_starts']
    assert st.shape == (4, 2) and np.all(np.diff(np.sort(st.ravel())) > 600000) and st.max() < a['summary'][1]
    assert a['summary'][1] - st.max() < 700000
    assert np.all(np.diff(a['field_linelocs'][:, :262], axis=1) > 2000)
    b_line = _plain_run(tmp_path / 'b', 1)
    assert b_line['steps'] == 1 and len(b_line['checks']['step_ms']) == 1
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / 'b' / (k + '.npy')), equal_nan=True), k


def test_bench_refuses_stream_file_on_a_sharded_launch():
    env = dict(os.environ, WORLD_SIZE='2', RANK='0', LOCAL_RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--stream-file', '/tmp/x'],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and 'the NTSC capture workload' in r.stderr
