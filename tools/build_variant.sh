#!/bin/bash
# build_variant.sh TAG UNIT [hipcc flags...]: libsfx_TAG.so with one unit of csrc/units.txt (e.g. collide, host/eval) compiled
# under extra flags and every other unit taken from csrc/obj as csrc/build.sh left it (tuning / diagnostic experiments, e.g.
# `build_variant.sh count collide -DPEN_COUNT`); load it with SFX_LIB=libsfx_TAG.so
set -e
PKG="$(cd "$(dirname "${BASH_SOURCE[0]}")/../smplify-x-partial_amd" && pwd)"; HERE="$PKG/csrc"; TAG=$1; UNIT=$2; shift; shift
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
VOBJ="${TMPDIR:-/tmp}/${UNIT//\//_}_$TAG.o"
objs=(); found=
while read -r unit own; do
  if [ "$unit" == "$UNIT" ]; then
    found=1; objs+=("$VOBJ")
    $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $own "$@" -c "$HERE/$unit.hip" -o "$VOBJ"
  else objs+=("$HERE/obj/${unit//\//_}.o"); fi
done < <(grep -v -e '^#' -e '^$' "$HERE/units.txt")
[ -n "$found" ] || { echo "unknown unit $UNIT (see csrc/units.txt)"; exit 1; }
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$PKG/libsfx_$TAG.so" "${objs[@]}"
echo built $TAG
