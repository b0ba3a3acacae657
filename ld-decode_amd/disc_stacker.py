#!/usr/bin/env python3
"""Stack several decodes of one disc into a single .tbc on the MI355X (build-defined,
DESIGN.md section 7b): every pixel from the sources that had no dropout there, so only
what every source lost is left to conceal.

    python ld-decode_amd/disc_stacker.py [-p] [--mode median|mean|smart-mean] [--threshold T]
        [--min-sources M] [--by-index] [--start K] [--length N] [--conceal] [--chunk C]
        [--device D] -o out a b c ...

Reads a.tbc + a.json, b.tbc + b.json, ... as `lddecode.py --dropouts` writes them (up to 16
sources of one system; a .json without 'dropouts' has no runs) and writes out.tbc and
out.json.  Frames are matched by their VBI frame number (--by-index: by position in the
file); --start / --length cut the output to the frame numbers [K, K + N).  out.json holds,
per output frame, the lowest-index present source's record with the residual dropouts (what
every present source lost) and 'stack': {'framenr', 'sources'}.  --conceal conceals the
residual in the stacked frames, as `lddecode.py --conceal` would.

The .pcm is not stacked: take the audio of the source you prefer.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from ldgpu import stack as S  # noqa: E402


def parse(argv):
    p = argparse.ArgumentParser(prog='disc_stacker.py', description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('-p', '--pal', action='store_true', help='PAL sources (default NTSC)')
    p.add_argument('--mode', choices=S.MODES, default='smart-mean')
    p.add_argument('--threshold', type=int, default=S.DEFAULT_THRESHOLD,
                   help='smart-mean: candidates this far from the median count (uint16 units, default 3840)')
    p.add_argument('--min-sources', type=int, default=1, help='output only frames at least this many sources have')
    p.add_argument('--by-index', action='store_true', help='match frames by position, not by VBI frame number')
    p.add_argument('--start', type=int, default=None, help='first frame number (--by-index: position) to output')
    p.add_argument('--length', type=int, default=None, help='frame numbers to output from --start')
    p.add_argument('--conceal', action='store_true', help='conceal the residual dropouts in the stacked frames')
    p.add_argument('--chunk', type=int, default=16, help='frames per GPU call')
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--stats', action='store_true', help='print the wall-time split as one JSON line on stderr')
    p.add_argument('-o', '--output', required=True, help='writes <output>.tbc and <output>.json')
    p.add_argument('sources', nargs='*', help='each names <source>.tbc and <source>.json')
    return p.parse_args(argv)


def fail(msg):
    print('disc_stacker: ' + msg, file=sys.stderr)
    return 1


def main(argv=None):
    args = parse(sys.argv[1:] if argv is None else argv)
    system = 'PAL' if args.pal else 'NTSC'
    W, H = S.OUTW[system], S.FRAME_LINES[system]
    fbytes = W * H * 2
    if not 1 <= len(args.sources) <= S.MAX_SOURCES:
        return fail('%d sources given: 1 to %d are stacked' % (len(args.sources), S.MAX_SOURCES))
    if not 0 <= args.threshold <= 65535 or args.chunk < 1:
        return fail('--threshold is 0..65535, --chunk at least 1')
    metas = []
    for name in args.sources:
        for ext in ('.tbc', '.json'):
            if not os.path.isfile(name + ext):
                return fail('%s%s: no such file' % (name, ext))
        size = os.path.getsize(name + '.tbc')
        if size % fbytes:
            return fail('%s.tbc: %d bytes is not a whole number of %s frames (%d bytes each)' % (name, size, system, fbytes))
        with open(name + '.json') as fh:
            meta = json.load(fh)
        if len(meta) != size // fbytes:
            return fail('%s: %d frames in the .tbc, %d records in the .json' % (name, size // fbytes, len(meta)))
        metas.append(meta)
    frames, skipped = S.align(metas, by_index=args.by_index, start=args.start, length=args.length,
                              min_sources=args.min_sources)
    for name, sk in zip(args.sources, skipped):
        if sk['no_key'] or sk['repeated']:
            print('disc_stacker: %s: %d frames without a frame number and %d with a repeated one left out'
                  % (name, sk['no_key'], sk['repeated']), file=sys.stderr)
    # a record without a valid field of either parity: the source is not present for that frame
    frames = [(k, [i if i is not None and S.frame_fields(metas[s][i]) else None for s, i in enumerate(idx)])
              for k, idx in frames]
    frames = [(k, idx) for k, idx in frames if sum(i is not None for i in idx) >= max(1, args.min_sources)]
    if not frames:
        return fail('no output frame left after alignment')

    from ldgpu import native
    n_src = len(args.sources)
    ctx = native.Context(system, args.device, max_reads=1, max_frames=args.chunk)
    tbcs = [open(name + '.tbc', 'rb') for name in args.sources]
    t = {'read_s': 0.0, 'host_s': 0.0, 'conceal_s': 0.0, 'write_s': 0.0}
    warned, out_meta = set(), []
    t_all = time.perf_counter()
    tmp = args.output + '.tbc.tmp'
    try:
        with open(tmp, 'wb') as fout:
            for c0 in range(0, len(frames), args.chunk):
                chunk = frames[c0:c0 + args.chunk]
                n = len(chunk)
                t0 = time.perf_counter()
                present = np.array([[i is not None for i in idx] for _, idx in chunk], dtype=np.uint8)
                srcs = []
                for s in range(n_src):
                    if not present[:, s].any():
                        srcs.append(None)
                        continue
                    buf = np.zeros((n, H * W), dtype=np.uint16)
                    f = 0
                    while f < n:                     # one read per run of consecutive frames of the file
                        i0 = chunk[f][1][s]
                        if i0 is None:
                            f += 1
                            continue
                        e = f + 1
                        while e < n and chunk[e][1][s] == i0 + (e - f):
                            e += 1
                        tbcs[s].seek(i0 * fbytes)
                        got = tbcs[s].readinto(memoryview(buf[f:e]).cast('B'))
                        if got != (e - f) * fbytes:
                            raise S.StackError('%s.tbc: short read at frame %d' % (args.sources[s], i0))
                        f = e
                    srcs.append(buf)
                t1 = time.perf_counter()
                runs = np.zeros((n, n_src, 2, S.MAX_LINES, S.MAX_PER_LINE, 2), dtype=np.int16)
                counts = np.zeros((n, n_src, 2, S.MAX_LINES), dtype=np.int32)
                nrows = np.zeros((n, 2), dtype=np.int32)
                res_r = np.zeros((n, 2, S.MAX_LINES, S.MAX_PER_LINE, 2), dtype=np.int16)
                res_c = np.zeros((n, 2, S.MAX_LINES), dtype=np.int32)
                for f, (key, idx) in enumerate(chunk):
                    here = [s for s in range(n_src) if idx[s] is not None]
                    for s in here:
                        fr = S.frame_runs(metas[s][idx[s]], system, '%s frame %d: ' % (args.sources[s], idx[s]))
                        runs[f, s], counts[f, s] = fr[0], fr[1]
                        if s == here[0]:
                            nrows[f] = fr[2]
                        if not fr[3] and s not in warned:
                            warned.add(s)
                            print("disc_stacker: %s.json has fields without 'dropouts': taken as free of dropouts"
                                  % args.sources[s], file=sys.stderr)
                    res_r[f], res_c[f] = S.residual(runs[f, here], counts[f, here], W)
                    out_meta.append(S.output_record(metas[here[0]][idx[here[0]]], c0 + f, key, here, res_r[f], res_c[f]))
                t2 = time.perf_counter()
                out = ctx.stack_frames(srcs, present, runs, counts, mode=args.mode, threshold=args.threshold)
                t3 = time.perf_counter()
                if args.conceal:                     # after stacking, never before: only the residual
                    out = ctx.conceal_frames(out, res_r, res_c, nrows)
                t4 = time.perf_counter()
                fout.write(out.data)
                t5 = time.perf_counter()
                t['read_s'] += t1 - t0
                t['host_s'] += t2 - t1
                t['conceal_s'] += t4 - t3
                t['write_s'] += t5 - t4
        stats = ctx.stack_stats()
    except (S.StackError, native.LDGError, OSError) as e:
        if os.path.exists(tmp):
            os.unlink(tmp)
        return fail(str(e))
    finally:
        for fh in tbcs:
            fh.close()
        ctx.close()
    t0 = time.perf_counter()
    with open(args.output + '.json.tmp', 'w') as fh:
        fh.write(json.dumps(out_meta))
    os.replace(tmp, args.output + '.tbc')
    os.replace(args.output + '.json.tmp', args.output + '.json')
    t['write_s'] += time.perf_counter() - t0
    if args.stats:
        t.update(stats, frames=len(frames), sources=n_src, wall_s=time.perf_counter() - t_all)
        print(json.dumps(t), file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
