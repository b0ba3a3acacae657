"""FLAC-compressed captures (.ldf, .flac, .oga), decoded on the GPU (ldg_flac_* of include/ldgpu.h;
build-defined).

    with FlacFile(ctx, 'side1.ldf') as f:      # opens and indexes
        f.nsamples, f.fmt, f.info, f.counters, f.gaps
        f.read(first, n)                        # numpy int16 / uint8
        f.capture()                             # the samples become the context's resident capture
"""
import ctypes as C
import os

import numpy as np

from . import native
from .formats import FMT_S16

EXTENSIONS = ('ldf', 'flac', 'oga')


def is_flac_path(path):
    """A file this project treats as FLAC: by extension (then ldg_flac_open by its first bytes)."""
    return path.rsplit('.', 1)[-1].lower() in EXTENSIONS


class FlacFile:
    def __init__(self, ctx, path, chunk_bytes=0, index=True):
        self.ctx, self.lib, self.path = ctx, ctx.lib, path
        info = native.FlacInfo()
        ctx._check(self.lib.ldg_flac_open(ctx.h, os.fsencode(path), C.byref(info)), 'ldg_flac_open')
        self.open = True
        self.info = {k: getattr(info, k) for k, _ in native.FlacInfo._fields_ if k not in ('pad_', 'md5')}
        self.info['md5'] = bytes(info.md5).hex()
        self.fmt = info.fmt
        self.dtype = np.dtype('<i2') if info.fmt == FMT_S16 else np.dtype(np.uint8)
        self.counters, self.nsamples = None, None
        if index:
            self.index(chunk_bytes)

    def index(self, chunk_bytes=0):
        """ldg_flac_index: scan, walk and keep over the whole file.  Returns the counters."""
        c = native.FlacCounters()
        self.ctx._check(self.lib.ldg_flac_index(self.ctx.h, int(chunk_bytes), C.byref(c)), 'ldg_flac_index')
        self.counters = {k: getattr(c, k) for k in native.FLAC_COUNTERS}
        self.nsamples, self.nframes = c.nsamples, c.frames
        return self.counters

    def tables(self):
        """(frames, gaps): the accepted frames as an array of native.FLAC_FRAME in byte order and the
        gaps as an int64 [n, 2] array of (first, count)."""
        frames = np.zeros(max(self.nframes, 1), dtype=native.FLAC_FRAME)
        gaps = np.zeros((max(self.counters['gaps'], 1), 2), dtype=np.int64)
        self.ctx._check(self.lib.ldg_flac_frames(self.ctx.h, frames.ctypes.data, self.nframes, gaps.ctypes.data,
                                                 self.counters['gaps']), 'ldg_flac_frames')
        return frames[:self.nframes], gaps[:self.counters['gaps']]

    @property
    def gaps(self):
        return [(int(a), int(b)) for a, b in self.tables()[1]]

    def read(self, first=0, n=None, out=None):
        """ldg_flac_read into host memory: samples [first, first + n) in the stream's format."""
        n = self.nsamples - first if n is None else n
        out = np.empty(n, dtype=self.dtype) if out is None else out
        assert out.dtype == self.dtype and out.size >= n and out.flags.c_contiguous
        self.ctx._check(self.lib.ldg_flac_read(self.ctx.h, int(first), int(n), out.ctypes.data, 0), 'ldg_flac_read')
        return out[:n]

    def read_device(self, first, n, device_ptr):
        self.ctx._check(self.lib.ldg_flac_read(self.ctx.h, int(first), int(n), C.c_void_p(device_ptr), 1),
                        'ldg_flac_read')

    def capture(self, first=0, n=None):
        """ldg_flac_capture: decode into a buffer the library owns and make it the resident capture."""
        n = self.nsamples - first if n is None else n
        self.ctx._check(self.lib.ldg_flac_capture(self.ctx.h, int(first), int(n)), 'ldg_flac_capture')
        return n

    def close(self):
        if self.open and self.ctx.h:
            self.lib.ldg_flac_close(self.ctx.h)
        self.open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
