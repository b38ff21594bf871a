#!/bin/bash
# Build an experimental libm3s variant: build_variant.sh NAME "-DMACRO=..."  ->  lightweight-mast3r-slam_amd/lib/exp/libm3s_NAME.so
# (load it with M3S_LIB=...; the shipped library is always csrc/Makefile's ../lib/libm3s.so). The variant is
# csrc/Makefile's own library target with the flags appended to every HIP compile, in an object directory of its own
# (csrc/build/exp/NAME): the object list and the per-file flags are the Makefile's.
set -e
cd "$(dirname "$0")/../lightweight-mast3r-slam_amd/csrc"
make -s -j8 BUILD="build/exp/$1" OUT="../lib/exp/libm3s_$1.so" EXTRA="$2" "../lib/exp/libm3s_$1.so"
echo built ../lib/exp/libm3s_$1.so
