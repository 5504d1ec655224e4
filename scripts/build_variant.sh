#!/bin/bash
# Build a measurement variant of the library next to the product build (never loaded unless G3_LIB_PATH names it):
#   scripts/build_variant.sh diag all -DG3_DIAG_TIMING                      -> g3py_amd/lib/libg3hip_diag.so
#   scripts/build_variant.sh w4 g3_chainb.hip -DG3_COOP_WAVES=4             -> g3py_amd/lib/libg3hip_w4.so
#   scripts/build_variant.sh v128 g3_potrf.hip -DG3_SMALL_VGPR=128          -> g3py_amd/lib/libg3hip_v128.so
# usage: build_variant.sh <name> <source file to recompile | all> <extra hipcc flags...>
# (`all` recompiles every translation unit: needed when the flags change something the units share.)  The translation
# units are the Makefile's SRCS.  Variant .so files are scratch: git ignores them.
set -e
name=$1; src=$2; shift 2
R=$(cd "$(dirname "$0")/.." && pwd)
make -C $R/g3py_amd/csrc -j4 > /dev/null
srcs=$(sed -n 's/^SRCS *:= *//p' $R/g3py_amd/csrc/Makefile)
[ -n "$srcs" ] || { echo "no SRCS in $R/g3py_amd/csrc/Makefile" >&2; exit 1; }
objs=""
for s in $srcs; do
  f=${s%.hip}
  if [ "$s" == "$src" ] || [ "$src" == "all" ]; then
    obj=/tmp/g3_variant_${name}_$f.o
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -I$R/include -Wall -Wno-unused-function -Wno-pass-failed "$@" -c $R/g3py_amd/csrc/$s -o $obj
    objs="$objs $obj"
  else
    objs="$objs $R/g3py_amd/lib/$f.o"
  fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/g3py_amd/lib/libg3hip_$name.so $objs -ldl
echo $R/g3py_amd/lib/libg3hip_$name.so
