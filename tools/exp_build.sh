#!/bin/bash
# Build an experimental variant of libstereo_amd.so (kernel A/B experiments; load it with SA_NATIVE_LIB=<path>).
# The kernel sources in SRC (one file, or a space-separated list) are recompiled -- with extra -D flags, or a single
# one replaced by another file -- and everything else links the normal objects.
#   bash tools/exp_build.sh <name> [-DSA_EXP_FOO ...]                      (variant of conv2d.hip)
#   SRC="csrc/kernels/conv2d.hip csrc/kernels/motion_enc.hip" bash tools/exp_build.sh <name> -DFOO   (both with -DFOO)
#   SRC=csrc/kernels/motion_enc.hip ALT=/tmp/old.hip bash tools/exp_build.sh <name>   (ALT compiled in SRC's place)
set -eo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
name=$1; shift
SRC=${SRC:-csrc/kernels/conv2d.hip}
out="$ROOT/stereoalgorithms_amd/lib/exp"
mkdir -p "$out" "$ROOT/build/exp"
objs=$(ls "$ROOT"/build/obj/dev/*.o)
new=""
for src in $SRC; do
  base=$(basename "$src")
  obj="$ROOT/build/exp/${base%.hip}_$name.o"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -x hip -O3 -std=c++17 -fPIC -I"$ROOT/csrc/include" -I"$ROOT/csrc/models" \
    -munsafe-fp-atomics "$@" -c "${ALT:-$ROOT/$src}" -o "$obj"
  objs=$(echo "$objs" | grep -v "/$base.o")
  new="$new $obj"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o "$out/libstereo_amd_$name.so" $objs $new \
  -L"$ROOT/stereoalgorithms_amd/lib" -lstereo_host -Wl,-rpath,'$ORIGIN/..' -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib
echo "$out/libstereo_amd_$name.so"
