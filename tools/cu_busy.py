"""Per-kernel sums of a tools/profile.sh PMC pass: CU-busy cycles against the demod's, VALU
instructions and waves (DESIGN.md sections 6g, 6k).

    python tools/cu_busy.py PROF/<tag>/pmc1/run_counter_collection.csv      (PROF: tools/profile.sh's output directory)

The pass must hold SQ_BUSY_CU_CYCLES, SQ_INSTS_VALU and SQ_WAVES (bench.py --no-cpu --steps 3
--warmup 1 in the committed tables)."""
import collections
import csv
import sys


def table(path):
    agg = collections.defaultdict(lambda: collections.defaultdict(float))
    disp = collections.defaultdict(set)
    for row in csv.DictReader(open(path)):
        k = row['Kernel_Name'].replace('(anonymous namespace)::', '').split('(')[0]
        agg[k][row['Counter_Name']] += float(row['Counter_Value'])
        disp[k].add(row['Dispatch_Id'])
    return agg, disp


def main(path):
    agg, disp = table(path)
    d = agg['ldg_k_demod']['SQ_BUSY_CU_CYCLES']
    print('%-28s %5s %12s %8s %12s %11s %10s' % ('kernel', 'disp', 'busy CU cyc', 'x demod', 'INSTS_VALU', 'WAVES', 'VALU/wave'))
    for k, v in sorted(agg.items(), key=lambda kv: -kv[1]['SQ_BUSY_CU_CYCLES']):
        w = v['SQ_WAVES']
        print('%-28s %5d %12.4g %8.3f %12.4g %11.4g %10.1f' % (k[:28], len(disp[k]), v['SQ_BUSY_CU_CYCLES'], v['SQ_BUSY_CU_CYCLES'] / d,
                                                              v['SQ_INSTS_VALU'], w, v['SQ_INSTS_VALU'] / w if w else 0))
    pipe = [k for k in agg if k.startswith('ldg_k_') and not k.startswith(('ldg_k_demod', 'ldg_k_synth', 'ldg_k_clock'))]
    print('non-demod pipeline kernels together: %.3f x the demod' % (sum(agg[k]['SQ_BUSY_CU_CYCLES'] for k in pipe) / d))


if __name__ == '__main__':
    main(sys.argv[1])
