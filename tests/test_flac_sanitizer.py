"""The FLAC-compressed captures' host logic (csrc/flac_plan.hpp: container, Ogg page walk, frame
header, keep / place bookkeeping) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/flac_san.cpp, a stand-alone program (no device, no library, nothing loaded into Python),
built here and run once over a valid native file, a valid Ogg file and 2,000 seeded mutations of
each.  Any report fails the run."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, 'oracle', '_build', 'san')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:halt_on_error=1',
           UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


def compiler():
    for c in ('/opt/rocm/llvm/bin/clang++', shutil.which('g++'), shutil.which('clang++')):
        if c and os.path.exists(c):
            return c
    return None


def test_flac_planning_clean_under_asan_ubsan():
    cxx = compiler()
    if cxx is None:
        pytest.skip('no C++ compiler')
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, 'flac_san')
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror'] + SAN + ['-o', exe, os.path.join(HERE, 'san', 'flac_san.cpp')],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=ENV)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert 'flac_san ok' in r.stdout
    for bad in ('AddressSanitizer', 'LeakSanitizer', 'runtime error:', 'FAIL'):
        assert bad not in out, out[-4000:]
