"""Counters of the benchmarked step kernel, collected with nothing else beside them:

    python tools/pmc_bench.py OUT.json [--tree DIR] [--steps 200] [--warmup 10]

ONE `rocprofv3 --pmc` pass (no tracing of any kind in the same run) of `bench.py --steps K --warmup W` in DIR (default: this
checkout; another checkout -- the parent commit's, built -- to compare).  Writes the means per launch over the LAST K dispatches of
k_step2, i.e. the timed steps, after the handle's plan is final (the plan's trial launches come first), the bench line of that run
(slower than an unprofiled one: the profiler serialises the launches), and the ratio SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU (busy
count per VALU instruction)."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ['SQ_INSTS_VALU', 'SQ_ACTIVE_INST_VALU', 'SQ_WAIT_INST_ANY', 'SQ_BUSY_CYCLES', 'GRBM_GUI_ACTIVE']


def main():
    args = sys.argv[1:]
    out = os.path.abspath(args[0])
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d
    tree, steps, warmup = os.path.abspath(opt('--tree', ROOT)), int(opt('--steps', 200)), int(opt('--warmup', 10))
    with tempfile.TemporaryDirectory() as d:
        res = subprocess.run(['rocprofv3', '--pmc'] + COUNTERS + ['--output-format', 'csv', '-d', d, '-o', 'pmc', '--',
                              sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)],
                             cwd=tree, capture_output=True, text=True, timeout=900)
        line = next((l for l in res.stdout.splitlines()[::-1] if l.startswith('{')), '')
        if res.returncode != 0 or not line:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-2000:])
            return 1
        rows = {}
        for fn in glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True):
            for row in csv.DictReader(open(fn)):
                if 'k_step2' in row['Kernel_Name']:
                    rows.setdefault(int(row['Dispatch_Id']), {})[row['Counter_Name']] = float(row['Counter_Value'])
    ids = sorted(rows)[-steps:]
    means = {c: sum(rows[i].get(c, 0.0) for i in ids) / len(ids) for c in COUNTERS}
    result = {'k_step2_dispatches_seen': len(rows), 'dispatches_averaged': len(ids), 'means_per_launch': means,
              'valu_cycles_per_instruction': means['SQ_ACTIVE_INST_VALU'] / max(1.0, means['SQ_INSTS_VALU']),
              'bench_line_under_the_profiler': json.loads(line)}
    json.dump(result, open(out, 'w'), indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in result.items() if k != 'bench_line_under_the_profiler'}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
