#!/bin/bash
# rocprofv3 evidence for profiles/: kernel-trace stats of the bench command, then the HBM-side counters of
# every gemm_w4a4 dispatch of the same command (separate --pmc passes, MI355X_MICROARCH.md "HBM").
# The command is bench.py --full: its dispatches include the instrumented and per-kernel steps behind the timed region.
#   usage: tools/gpu_profile_bench.sh OUTDIR
O=$(realpath -m "${1:?usage: tools/gpu_profile_bench.sh OUTDIR}")
mkdir -p "$O"
export TMPDIR=/tmp
R=$PWD
cd /tmp
# each pass has its own time limit; a pass that fails, faults or hangs ends the script before the next one starts on the card
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o bench -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > "$O/trace.log" 2>&1 &&
timeout -k 10 900 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$O/fetch" -o g -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$O/fetch.log" 2>&1 &&
timeout -k 10 900 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$O/write" -o g -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline > "$O/write.log" 2>&1 ||
  { rc=$?; echo "a rocprofv3 pass failed (exit $rc): see $O/*.log" >&2; exit $rc; }
cd $R
grep -h '"metric"' "$O/trace.log" | head -1
python - "$O" <<'PY'
import csv, glob, collections, json, sys
O = sys.argv[1]
for f in glob.glob(f'{O}/trace/**/*kernel_stats.csv', recursive=True):
    rows=list(csv.DictReader(open(f)))
    for r in rows[:8]: print({k:(v[:60] if k=='Name' else v) for k,v in r.items() if k in ('Name','Calls','AverageNs','Percentage')})
out={}
for d in ('fetch','write'):
    for f in glob.glob(f'{O}/{d}/**/*counter_collection.csv', recursive=True):
        agg=collections.defaultdict(list)
        for r in csv.DictReader(open(f)):
            if 'gemm_w4a4' in r['Kernel_Name']:
                agg[(r['Counter_Name'])].append(float(r['Counter_Value']))
        for k,v in agg.items():
            print(d,k,'avg per gemm dispatch',sum(v)/len(v), 'n',len(v)); out[k]={'avg_per_dispatch_KB':sum(v)/len(v),'dispatches':len(v)}
json.dump(out, open(f'{O}/gemm_hbm_counters.json','w'), indent=1)
PY
# keep the big raw traces out of the evidence: only stats + summaries
find "$O" -name "*kernel_trace.csv" -delete
find "$O" -name "*counter_collection.csv" -size +8M -delete
