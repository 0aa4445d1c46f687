#!/bin/bash
# Builds kernel variants for A/B timing into build/ (git-ignored, travels to the GPU box).  usage: build_variants.sh name "-DFLAG ..." ...
set -e
cd "$(dirname "$0")/.."
while [ $# -gt 0 ]; do
  name=$1; flags=$2; shift 2
  mkdir -p build
  python gym_sbr2_amd/build.py -o build/libsbr_amd_$name.so $flags      # the library's own flags and units, $flags behind them
  echo "built build/libsbr_amd_$name.so  [$flags]"
done
