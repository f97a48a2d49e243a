#!/bin/bash
# PMC passes over the bench workload (one counter group per run; never combined with tracing).
# usage: profiles/pmc_passes.sh <outdir-under-gpurun_out> [bench args...]
set -u
BENCH=$(cd "$(dirname "$0")/.." && pwd)/bench.py
OUT=$GRAFT_REPO_ROOT/gpurun_out/$1; shift
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
run() { # name counters...
  name=$1; shift
  rocprofv3 --pmc "$@" --output-format csv -d $OUT/$name -- python3 $BENCH --steps 4 --warmup 1 --full --no-cpu-baseline $BENCH_ARGS > $OUT/$name.json 2> $OUT/$name.err || echo "pass $name failed"
}
BENCH_ARGS="$*"
run fetch FETCH_SIZE
run write WRITE_SIZE
run tcc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum
run sq1 SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU
run sq2 SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INST_CYCLES_VMEM SQ_WAIT_INST_LDS
run tcp TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum
run grbm GRBM_GUI_ACTIVE
ls -R $OUT | head -40
