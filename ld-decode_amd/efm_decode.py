#!/usr/bin/env python3
"""EFM run lengths to 44.1 kHz PCM (F3 frames, CIRC), on the MI355X.

    python ld-decode_amd/efm_decode.py [--efm-table F] [--chunk-bytes N] [--stats] [--data] in.efm out

Reads a .efm file (one byte per run length, as efm_extract.py and lddecode.py --efm write
them) and writes <out>.efm.pcm -- s16le stereo at 44.1 kHz -- and <out>.efm.pcm.json: frames,
samples, sync candidates / confirmed, coasted frames, breaks, bad symbols, the C1 and C2
outcomes, flagged / averaged / muted samples and the subcode Q figures (sections, good CRCs,
first and last time code).  The rule is this project's own (BUILD-DEFINED, DESIGN.md section
7d): parity with a real player is not pinned.  The code table is read from
tests/golden/efm_map.txt of this repository, or from --efm-table.

--data: the channel carries CD-ROM mode 1 sectors instead of sound.  Also writes <out>.efm.data --
the 2048 user bytes of every sector found, in grid order -- and <out>.efm.data.json: sectors, sync
candidates / confirmed, coasted, breaks, good / corrected / bad / other sectors, P and Q words
fixed, erased bytes, the first and last address, the address discontinuities and the first 1000
bad sectors.  The bytes are taken before concealment, each erased by its own C2 flag, and a
sector the EDC does not verify is passed on without any Reed-Solomon change (BUILD-DEFINED,
DESIGN.md section 7e: parity with a real drive is not pinned).  The other outputs do not change.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from ldgpu import efmdec, efmsec, native  # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser(description='Decodes EFM run lengths to 44.1 kHz PCM')
    p.add_argument('efm', help='source file: one byte per run length')
    p.add_argument('out', help='base name: <out>.efm.pcm and <out>.efm.pcm.json')
    p.add_argument('--efm-table', default=None,
                   help='the code table: 256 lines of 14 channel bits, value 0 first (default: tests/golden/efm_map.txt)')
    p.add_argument('--chunk-bytes', type=int, default=1 << 24, help='run lengths per GPU call (the output does not depend on it)')
    p.add_argument('--stats', action='store_true', help='add wall time and per-kernel times to the .efm.pcm.json')
    p.add_argument('--data', action='store_true',
                   help='also decode CD-ROM mode 1 sectors: <out>.efm.data (2048 bytes a sector) and <out>.efm.data.json')
    p.add_argument('--device', type=int, default=0, help='HIP device')
    return p.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if args.chunk_bytes < 1:
        print('ERROR: --chunk-bytes must be at least 1')
        return 1
    try:
        efmdec.load_table(args.efm_table)
    except (OSError, ValueError) as e:
        print('ERROR: %s' % e)
        return 1
    ctx = native.Context('NTSC', args.device, max_reads=1)
    try:
        if args.data:
            summ, dsumm = efmsec.decode_file(ctx, args.efm, args.out, args.chunk_bytes, args.efm_table, stats=args.stats)
            summ = dict(summ, data=dsumm)
        else:
            summ = efmdec.decode_file(ctx, args.efm, args.out, args.chunk_bytes, args.efm_table, stats=args.stats)
    finally:
        ctx.close()
    print(json.dumps(summ))
    return 0


if __name__ == '__main__':
    sys.exit(main())
