#!/bin/bash
# Builds a VARIANT of liblinearham_hip.so (extra compiler flags) into its own directory
# linearham_amd/lib_exp/<label>/ next to a copy of the host library (whose rpath is $ORIGIN), leaving the product
# library alone; LH_LIB_DIR=<that directory> makes linearham_amd/capi.py and host.py load it.
# usage (anywhere hipcc runs; the .so files travel to the GPU box): bash tools/build_variant.sh label "-DFOO -DBAR=2"
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
label=$1
flags=${2:-}
out=$root/linearham_amd/lib_exp/$label
mkdir -p "$out"
# the product library's source list (linearham_amd/build.py HIP_SOURCES)
mapfile -t srcs < <(cd "$root" && python3 -c "from linearham_amd.build import CSRC, HIP_SOURCES
import os
print('\n'.join(os.path.join(CSRC, s) for s in HIP_SOURCES))")
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-unused-result $flags -I "$root/include" -I "$root/linearham_amd/csrc" \
  "${srcs[@]}" -o "$out/liblinearham_hip.so"
cp "$root/linearham_amd/lib/liblinearham_host.so" "$out/"
echo "built $out ($flags)"
