#!/usr/bin/env python3
"""Unpack a FLAC-compressed capture (.ldf, .flac, .oga) to its raw samples on the GPU.

    ldf_unpack.py [--start-sample S --length L] [--md5] [--stats] in.ldf out.r16     (or out.u8)

The file goes through the frame index (ldg_flac_index) and ldg_flac_read, a piece at a time;
out.json (next to the output) holds the stream info, the counters and the gaps.  --md5 hashes the
unpacked samples on the host and compares them with the MD5 the encoder left in STREAMINFO: the one
tie to the encoder that made the file (a whole-capture unpack with a non-zero MD5 only)."""
import argparse
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from ldgpu import native  # noqa: E402
from ldgpu.flac import FlacFile  # noqa: E402
from ldgpu.formats import FMT_S16  # noqa: E402

PIECE = 1 << 25                      # samples a read


def parse(argv=None):
    p = argparse.ArgumentParser(description='Unpack a FLAC-compressed LaserDisc capture on the GPU')
    p.add_argument('infile')
    p.add_argument('outfile')
    p.add_argument('--start-sample', type=int, default=0)
    p.add_argument('--length', type=int, default=None, help='samples to unpack (default: to the end)')
    p.add_argument('--md5', action='store_true', help="compare the samples' MD5 with STREAMINFO's")
    p.add_argument('--stats', action='store_true', help='print the counters and the pace')
    p.add_argument('--chunk-mb', type=int, default=0, help='file bytes an index launch takes (default 64)')
    p.add_argument('--device', type=int, default=0)
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    ctx = native.Context('NTSC', args.device, max_reads=1)
    t0 = time.perf_counter()
    try:
        f = FlacFile(ctx, args.infile, chunk_bytes=args.chunk_mb << 20)
    except native.LDGError as e:
        print('ERROR: %s' % e)
        return 1
    t_index = time.perf_counter() - t0
    want_ext = '.r16' if f.fmt == FMT_S16 else '.u8'
    if not args.outfile.lower().endswith(want_ext):
        print('note: the samples are %s; the output is written as given (%s)' % (want_ext[1:], args.outfile))
    first = args.start_sample
    n = f.nsamples - first if args.length is None else args.length
    if first < 0 or n < 0 or first + n > f.nsamples:
        print('ERROR: samples [%d, %d) are not within the capture\'s %d' % (first, first + n, f.nsamples))
        return 1
    whole = first == 0 and n == f.nsamples
    md5 = hashlib.md5() if args.md5 else None
    buf = np.empty(min(PIECE, max(n, 1)), dtype=f.dtype)
    t1 = time.perf_counter()
    with open(args.outfile, 'wb') as out:
        for at in range(first, first + n, PIECE):
            piece = f.read(at, min(PIECE, first + n - at), out=buf)
            out.write(piece)
            if md5 is not None:         # FLAC's MD5 is of the signed samples, little-endian
                md5.update(piece if f.fmt == FMT_S16 else (piece ^ 0x80))
    t_read = time.perf_counter() - t1
    verdict = None
    if args.md5:
        if not whole:
            verdict = 'not checked: --md5 needs the whole capture'
        elif int(f.info['md5'], 16) == 0:
            verdict = 'not checked: STREAMINFO carries no MD5'
        elif f.counters['gaps'] == 0 and md5.hexdigest() == f.info['md5']:
            verdict = 'match'
        else:
            verdict = 'MISMATCH: unpacked %s, STREAMINFO %s' % (md5.hexdigest(), f.info['md5'])
        print('md5: %s' % verdict)
    info = dict(f.info, nsamples=f.nsamples, first_sample=first, length=n, counters=f.counters, gaps=f.gaps,
                md5_verdict=verdict)
    with open(os.path.splitext(args.outfile)[0] + '.json', 'w') as fh:
        json.dump(info, fh, indent=1)
    if args.stats:
        print(json.dumps(f.counters))
        print('index %.2f s, unpack of %d samples %.2f s (%.0f Msamples/s with the write)' % (
            t_index, n, t_read, n / max(t_read, 1e-9) / 1e6))
    f.close()
    ctx.close()
    return 1 if verdict is not None and verdict.startswith('MISMATCH') else 0


if __name__ == '__main__':
    sys.exit(main())
