#!/bin/bash
# same-box A/B of the whole denoise step: an earlier commit's tree, built, vs this tree.  Prepare the earlier tree with
#   mkdir -p DIR && git archive <rev> | tar -x -C DIR && (cd DIR && python -m nunchaku_amd.build)
#   usage: tools/gpu_ab_step.sh DIR
OLD="${1:?usage: tools/gpu_ab_step.sh DIR_OF_AN_EARLIER_BUILT_TREE}"
# the roofline object needs --full (a bench.py older than that option always measured it)
OLD_FULL=$(grep -q -- '"--full"' "$OLD/bench.py" && echo --full)
P='import sys,json; r=json.loads(sys.stdin.read()); ro=r["roofline"]; print("%.2f ms/step  gemm %.2f ms (frac %.3f)  quant %.2f  attn %s" % (r["ms_per_step"], ro["gemm_ms_per_step"], ro["frac"], ro["quantize"]["ms_per_step"], ro.get("attention",{}).get("ms_per_step")))'
# each run has its own time limit; the first run that fails, faults or hangs ends the script before the next one starts on the card
set -o pipefail
for rep in 1 2; do
  echo -n "old: "; (cd "$OLD" && timeout -k 10 600 python bench.py $OLD_FULL --steps 20 --warmup 3 --no-prof 2>/dev/null | tail -1 | python -c "$P") || exit
  echo -n "new: "; timeout -k 10 600 python bench.py --full --steps 20 --warmup 3 --no-prof 2>/dev/null | tail -1 | python -c "$P" || exit
done
