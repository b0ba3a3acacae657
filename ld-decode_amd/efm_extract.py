#!/usr/bin/env python3
"""EFM (digital audio) run lengths of an RF capture, on the MI355X.

    python ld-decode_amd/efm_extract.py [--start-sample S --end-sample E] [--chunk-segments C]
                                        [--stats] capture out

Writes <out>.efm -- one byte per run length between the EFM signal's zero crossings, 3..11
channel bits, the input of efm_decode.py (F3 frames, CIRC, 44.1 kHz PCM; DESIGN.md section
7d) -- and <out>.efm.json, a summary with the one check that needs no code table: how
many consecutive sync patterns (11, 11) lie 588 channel bits apart.  The rule is this
project's own (BUILD-DEFINED).  The sample range is widened outward to
whole segments of 2^20 samples.  Loader selection by extension as lddecode.py.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from ldgpu import efm, native  # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser(description='Extracts the EFM run lengths from raw RF laserdisc captures')
    p.add_argument('capture', help='source file (.lds / .r30 / .r16, else 8-bit)')
    p.add_argument('out', help='base name: <out>.efm and <out>.efm.json')
    p.add_argument('--start-sample', type=int, default=0, help='first RF sample (default 0)')
    p.add_argument('--end-sample', type=int, default=None, help='one past the last RF sample (default: the end)')
    p.add_argument('--chunk-segments', type=int, default=64, help='segments of 2^20 samples per GPU call')
    p.add_argument('--stats', action='store_true', help='add wall time and per-kernel times to the .efm.json')
    p.add_argument('--device', type=int, default=0, help='HIP device')
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if args.chunk_segments < 1:
        print('ERROR: --chunk-segments must be at least 1')
        return 1
    if args.end_sample is not None and args.end_sample < args.start_sample:
        print('ERROR: --end-sample lies before --start-sample')
        return 1
    ctx = native.Context('NTSC', args.device, max_reads=1)
    try:
        summ = efm.extract_file(ctx, args.capture, args.out, args.start_sample, args.end_sample, args.chunk_segments,
                                stats=args.stats)
    finally:
        ctx.close()
    print(json.dumps(summ))
    return 0


if __name__ == '__main__':
    sys.exit(main())
