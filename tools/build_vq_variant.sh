#!/bin/bash
# dev: variant libraries that differ only in cgic_vq.hip (an edited constant, extra flags): that unit is recompiled, the others are
# linked from the objects `make` leaves in csrc/ (`make vq-variant`: sources and flags are the Makefile's).
# usage: tools/build_vq_variant.sh name1 "" name2 "-DCGIC_PHASE_CLOCKS" ...   -> tmp_libs/lib_<name>.so
set -e
cd "$(dirname "$0")/../control-gic_amd/csrc"
while [ $# -ge 2 ]; do
  name=$1; extra=$2; shift 2
  ( make -s vq-variant NAME="$name" EXTRA="$extra" && echo built $name ) &
done
wait
