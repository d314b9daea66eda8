#!/bin/bash
# Developer tool: instruction-cache and instruction-issue counters of the bench kernel, in counter passes of their OWN (rocprofv3 --pmc with no
# tracing option; the collection's CSV names the kernel of every dispatch by itself). Run on a GPU box from the repository root:
#   tests/tools_pmc_icache_only.sh TAG [LIB]     LIB: another build of the library (PMPC_LIB), e.g. polympc_amd/_variants/lib_parent.so
# Output: $PMC_OUT/pmc_TAG_{ic,issue}/ and $PMC_OUT/TAG_icache_pmc_summary.json (per-launch means of the headline kernel, library_build_id); PMC_OUT defaults to build/pmc.
# The counter names are checked against the tool's own list first: a name the device does not offer is left out of its pass and reported.
# Every GPU step runs under a time limit of its own and the steps are chained: nothing starts after one that failed.
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r11}
LIB=${2:-}
[ -n "$LIB" ] && export PMPC_LIB=$(cd "$(dirname "$LIB")" && pwd)/$(basename "$LIB")
export PMC_OUT=${PMC_OUT:-$R/build/pmc}
OUT=$PMC_OUT
mkdir -p $OUT
cd $R
BENCH="python $R/bench.py --gpus 1 --steps 5 --warmup 1 --detail-out="
timeout -k 10 120 rocprofv3 -L > $OUT/pmc_${TAG}_counter_list.txt 2>&1 || { echo "rocprofv3 -L failed"; tail -3 $OUT/pmc_${TAG}_counter_list.txt; exit 1; }
avail() { for c in "$@"; do if grep -qw "$c" $OUT/pmc_${TAG}_counter_list.txt; then printf "%s " $c; else echo "not offered by this device: $c" >&2; fi; done; }
IC=$(avail SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQ_IFETCH SQ_WAIT_INST_ANY SQ_WAVE_CYCLES)
ISSUE=$(avail SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_ANY)
echo "pass ic: $IC"; echo "pass issue: $ISSUE"
run() { name=$1; shift; timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d $OUT/pmc_${TAG}_$name -o $name -- $BENCH > $OUT/pmc_${TAG}_$name.log 2>&1; }
run ic $IC && run issue $ISSUE && timeout 60 python $R/tests/tools_pmc_icache_summary.py $TAG
st=$?
[ $st -ne 0 ] && { echo "stopped with status $st"; tail -5 $OUT/pmc_${TAG}_ic.log $OUT/pmc_${TAG}_issue.log 2>/dev/null; }
exit $st
