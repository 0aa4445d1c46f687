#!/bin/bash
# Instruction-fetch counters of k_step over whole episodes of the bench workload at 65 536 envs (profiles/r22_notes.md):
# two rocprofv3 --pmc passes, counters ONLY (no tracing in the same run), each a process of its own.
#   pass sq:   SQ_WAIT_INST_ANY SQ_IFETCH SQ_WAVE_CYCLES SQ_BUSY_CYCLES (+ SQ_WAVES, SQ_WAIT_ANY, SQ_INSTS_VALU for the per-wave figures)
#   pass sqc:  the instruction-cache counters of the scalar cache block (request, hit, miss, duplicate miss, requests to L2)
# usage: bash scripts/probes/pmc_ifetch.sh <outdir> [library]      then: python scripts/probes/pmc_ifetch_summary.py <outdir>
set -e -o pipefail
out=${1:-build/pmc_ifetch}
if [ -n "$2" ]; then export SBR_AMD_LIB=$2; else unset SBR_AMD_LIB; fi
mkdir -p $out
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
export PMC_ENVS=65536
timeout -k 10 240 rocprofv3 --pmc SQ_WAIT_INST_ANY SQ_IFETCH SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES SQ_WAIT_ANY SQ_INSTS_VALU \
  -d $out/sq -o run --output-format csv -- python3 scripts/pmc_workload.py > $out/sq.json 2> $out/sq.err
echo "SQ pass done"
timeout -k 10 240 rocprofv3 --pmc SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE SQC_TC_INST_REQ SQ_WAVES \
  -d $out/sqc -o run --output-format csv -- python3 scripts/pmc_workload.py > $out/sqc.json 2> $out/sqc.err
echo "SQC pass done"
python3 scripts/probes/pmc_ifetch_summary.py $out | tee $out/summary.txt
# the raw per-dispatch tables are large: the summary is what is kept
rm -rf $out/sq $out/sqc
