#!/bin/bash
# Build an alternative libemurx.so with extra compiler flags, for A/B runs (EMURX_LIB=...):
#   tools/build_variant.sh <name> "<-DFLAG=..>"   -> trex-emu_amd/lib/libemurx_<name>.so
# The Makefile's own sources and rules with the flags appended, the objects in build/var_<name>/;
# always from scratch (-B): the flags are no dependency of the objects.
set -eu
cd "$(dirname "$0")/../trex-emu_amd"
name=$1; flags=$2
make -s -B -j8 BUILD=build/var_$name LIBNAME=emurx_$name EXTRA="$flags" lib/libemurx_$name.so
echo lib/libemurx_$name.so
