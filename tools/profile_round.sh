#!/bin/bash
# Collects the round's profiles on a GPU box (run through gpurun from the repo root):
#   gpurun --timeout 1500 -- 'bash tools/profile_round.sh r02'
# Writes under gpurun_out/<tag>/ (merged back by gpurun); tools/summarize_profile.py turns them into profiles/<tag>_*.
# rocprofv3 rules of this pool: --pmc passes carry --kernel-trace only, one counter family per pass.
set -u
TAG=${1:-r02}
R=$PWD
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
# 1. the un-profiled bench line with every record (--full: the CPU baseline leg among them) + the per-shape GEMM table from its events
python $R/bench.py --full --steps 20 --warmup 5 --shape-log $OUT/gemm_shapes.json > $OUT/bench.json 2> $OUT/bench.err
# 2. per-kernel statistics.  The profiled command skips the render + settle phases (their kernels would swamp the table) and reaches
#    the timed regime directly (the coarse stage at the configuration's lr 1e-4); its own JSON line (kept) reports the converged
#    fraction it ran at.
PROF="python $R/bench.py --full --steps 30 --warmup 5 --settle 0 --settle-low 0 --noise-observations --no-fine --no-cpu-baseline --no-extra-records"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- $PROF > $OUT/stats.log 2>&1
python $R/tools/gap_analysis.py $OUT/stats 17 44 > $OUT/gaps.txt 2>&1            # GPU busy / idle of the clean pass (iterations 17..43 of 75) and where the idle time sits
python $R/tools/iteration_timeline.py $OUT/stats 45 > $OUT/timeline.txt 2>&1   # one iteration of the clean pass: segments of GPU activity and the gaps between them
find $OUT/stats -name "*kernel_trace.csv" -delete
# 3. HBM traffic of the layer GEMMs: FETCH_SIZE and WRITE_SIZE in separate passes, + the calibration launches
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/pmc_$C -- python $R/bench.py --full --steps 6 --warmup 0 --settle 0 --settle-low 0 --noise-observations --no-fine --no-cpu-baseline --no-extra-records --no-sdf-throughput --shape-log $OUT/pmc_shapes_$C.json > $OUT/pmc_$C.log 2>&1
  rocprofv3 --kernel-trace --pmc $C --output-format csv -d $OUT/cal_$C -- python $R/tools/pmc_calibrate.py > $OUT/cal_$C.log 2>&1
  python - "$OUT" "$C" <<'PY'
import csv, glob, sys, json, collections
out, c = sys.argv[1], sys.argv[2]
def collect(d, by_grid=False):
    agg = collections.defaultdict(lambda: [0, 0.0])
    for f in glob.glob(d + '/*/*counter_collection.csv'):
        for r in csv.DictReader(open(f)):
            if r['Counter_Name'] != c: continue
            n = r['Kernel_Name']
            if 'gemm_nt_kernel' in n:      # per tile configuration: <2,2,*,*> are the wide-output launches the shape log records
                key = 'gemm_nt_kernel' + n[n.index('<'):n.index('>') + 1].replace(' ', '')
            elif by_grid and ('elementwise_kernel' in n or 'copyBuffer' in n or 'CatArrayBatchedCopy' in n):
                key = 'stream_copy'                   # calibration pass only: torch's vectorised copy (tools/pmc_calibrate.py)
            else:
                key = 'gemm_tn_kernel' if 'gemm_tn_kernel' in n else 'mlp_layer_pair_kernel' if 'mlp_layer_pair_kernel' in n else None
            if not key: continue
            if by_grid: key = key + ' grid ' + r['Grid_Size']
            agg[key][0] += 1; agg[key][1] += float(r['Counter_Value'])
    return {k: {'launches': v[0], 'avg': v[1] / max(v[0], 1)} for k, v in agg.items()}
json.dump(collect(out + '/pmc_' + c), open(out + '/pmc_' + c + '.json', 'w'), indent=1)
json.dump(collect(out + '/cal_' + c, True), open(out + '/cal_' + c + '.json', 'w'), indent=1)
PY
  rm -rf $OUT/pmc_$C $OUT/cal_$C
done
# 4. kernel micro-benchmarks against their rooflines
python $R/tools/kernel_bench.py > $OUT/hbm_kernels.md 2> $OUT/hbm_kernels.err
python $R/tools/gemm_bench.py > $OUT/gemm_bench.txt 2>&1
cd $R
ls -la $OUT
