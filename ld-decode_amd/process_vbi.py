#!/usr/bin/env python3
"""The NTSC line services of an existing .tbc on the MI355X (build-defined, DESIGN.md section
7f): the white flag, the closed captions and the video ID of every field.

    python ld-decode_amd/process_vbi.py in.tbc [-o out] [--chunk C] [--device D] [--stats]

Reads the 910 x 525 frames of in.tbc (lddecode.py's output, or disc_stacker.py's) and writes
out.lines.json (default: beside the input, in.lines.json): {'frames': [{'frame': i, 'fields':
[top, bottom]}, ...], 'counts': {...}} with the fields' records as `lddecode.py --line-services`
writes them ('lineServices'), and counts of the white flags and of the fields per caption and
video ID state.  --stats prints the counts.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

W, H = 910, 525
STATES = ('absent', 'ok', 'check', 'frame')      # LDG_LINE_*


def parse(argv):
    p = argparse.ArgumentParser(prog='process_vbi.py', description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('tbc', help='the NTSC .tbc to read')
    p.add_argument('-o', '--output', default=None, help='writes <output>.lines.json (default: the input without .tbc)')
    p.add_argument('--chunk', type=int, default=64, help='frames per GPU call')
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--stats', action='store_true', help='print the counts')
    return p.parse_args(argv)


def fail(msg):
    print('process_vbi: ' + msg, file=sys.stderr)
    return 1


def count(records):
    """Counts over the fields' 'lineServices' records: white flags, and fields per state."""
    c = {'fields': len(records), 'white': sum(1 for r in records if r['white']),
         'cc': {s: 0 for s in STATES}, 'videoId': {s: 0 for s in STATES}}
    for r in records:
        c['cc'][STATES[r['ccState']]] += 1
        c['videoId'][STATES[r['videoIdState']]] += 1
    return c


def main(argv=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    fbytes = W * H * 2
    if not os.path.isfile(args.tbc):
        return fail('%s: no such file' % args.tbc)
    size = os.path.getsize(args.tbc)
    if size % fbytes:
        return fail('%s: %d bytes is not a whole number of NTSC frames (%d bytes each)' % (args.tbc, size, fbytes))
    if args.chunk < 1:
        return fail('--chunk is at least 1')
    out = args.output if args.output is not None else (args.tbc[:-4] if args.tbc.endswith('.tbc') else args.tbc)
    nframes = size // fbytes

    from ldgpu import native
    ctx = native.Context('NTSC', args.device, max_reads=1, max_frames=1)
    frames, flat = [], []
    try:
        buf = np.zeros((args.chunk, H * W), dtype=np.uint16)
        with open(args.tbc, 'rb') as fh:
            for f0 in range(0, nframes, args.chunk):
                n = min(args.chunk, nframes - f0)
                if fh.readinto(memoryview(buf[:n]).cast('B')) != n * fbytes:
                    return fail('%s: short read at frame %d' % (args.tbc, f0))
                for i, pair in enumerate(ctx.frames_line_services(buf[:n])):
                    recs = [native.line_services_json(r) for r in pair]
                    frames.append({'frame': f0 + i, 'fields': recs})
                    flat += recs
    except (native.LDGError, OSError) as e:
        return fail(str(e))
    finally:
        ctx.close()
    counts = count(flat)
    with open(out + '.lines.json.tmp', 'w') as fh:
        fh.write(json.dumps({'frames': frames, 'counts': counts}))
    os.replace(out + '.lines.json.tmp', out + '.lines.json')
    if args.stats:
        print(json.dumps(dict(counts, frames=nframes)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
