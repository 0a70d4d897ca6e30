#!/bin/bash
# dev: build variant libraries of the sources AS THEY STAND (an edited constant) with extra flags into tmp_libs/ (git-ignored);
# sources and flags are the Makefile's (`make variant`).  The A/B preprocessor switches these scripts once drove are gone:
# the last commit that has them is f0c5b5b.
# usage: tools/build_variants.sh name1 "" name2 "-DCGIC_PHASE_CLOCKS" ...
set -e
cd "$(dirname "$0")/../control-gic_amd/csrc"
while [ $# -ge 2 ]; do
  name=$1; extra=$2; shift 2
  ( make -s variant NAME="$name" EXTRA="$extra" && echo built $name ) &
done
wait
