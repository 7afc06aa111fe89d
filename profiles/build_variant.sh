#!/bin/bash
# Build an A/B variant of the library: bash profiles/build_variant.sh NAME UNIT "EXTRA FLAGS"
#   -> emd_amd/csrc/variants/lib_NAME.so = the in-tree objects with UNIT.hip recompiled with the extra -D flags (run `make -C emd_amd/csrc` first).
# The object list and every unit's flags come from the Makefile (print-objs, print-flags-UNIT).  The compile runs inside emd_amd/csrc: a relative path
# in EXTRA FLAGS (-I, -include) is taken from there, not from the caller's directory.
# Selected at run time with EMD_LIB_PATH (profiles/ab_variants.sh).
set -e
NAME=$1; UNIT=$2; EXTRA=$3
cd "$(dirname "$0")/../emd_amd/csrc"
mkdir -p variants
FLAGS=$(make -s --no-print-directory print-flags-$UNIT)
/opt/rocm/bin/hipcc $FLAGS $EXTRA -c $UNIT.hip -o variants/${UNIT}_$NAME.o 2> variants/${UNIT}_$NAME.log || { tail -20 variants/${UNIT}_$NAME.log; exit 1; }
OBJS=""
for o in $(make -s --no-print-directory print-objs); do
  if [ $o = $UNIT.o ]; then OBJS="$OBJS variants/${UNIT}_$NAME.o"; else OBJS="$OBJS $o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/lib_$NAME.so $OBJS
echo built emd_amd/csrc/variants/lib_$NAME.so
