#!/bin/bash
# Builds abl/<name>.so = the library with ONE source recompiled under extra compiler flags (A/B-ing a kernel variant
# inside one GPU session: pass it through MPSR_LIB_PATH).  The object is built by the Makefile's own rule for that
# source, so it carries the same per-file flags as the default build plus the extra ones.
# usage: tools/build_variant.sh <name> <source.hip> <flags...>
set -e
NAME=$1; SRC=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT/monopsr_amd/csrc"
make -s -j8
mkdir -p "$ROOT/abl"
O="${SRC%.hip}.o"
OBJ="$ROOT/abl/$NAME.$O"
make -s -B EXTRA="$*" "$O"
mv "$O" "$OBJ"
make -s "$O"  # the default object back in place
OTHERS=$(ls *.o | grep -v "^$O$")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/abl/$NAME.so" $OTHERS "$OBJ"
echo "built abl/$NAME.so"
