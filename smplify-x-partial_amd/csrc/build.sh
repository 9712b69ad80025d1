#!/bin/bash
# Build libsfx.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [outdir]
#   SFX_LAB=1 build.sh   builds libsfx_lab.so instead: the same sources with -DSFX_LAB -- the A/B forms, environment switches and
#                        phase clocks of include/sfx_lab.h (tools/, tools/run_gpu_suite.sh); the product library has none of them.
# The units and their own flags are listed once, in units.txt; at most min(16, MAX_JOBS) compile at a time.
# SFX_NAME / SFX_OBJ: another library name / object directory (tools/build_full_variant.sh).
set -e
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${1:-$HERE/..}"
export HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
NAME=libsfx.so; OBJ="$HERE/obj"
if [ -n "$SFX_LAB" ]; then NAME=libsfx_lab.so; OBJ="$HERE/obj_lab"; SFX_DEFINES="$SFX_DEFINES -DSFX_LAB"; fi
NAME="${SFX_NAME:-$NAME}"; OBJ="${SFX_OBJ:-$OBJ}"
export HERE OBJ FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $SFX_DEFINES"   # SFX_DEFINES: diagnostic -D switches (tools/)
mkdir -p "$OBJ"
JOBS="${MAX_JOBS:-16}"; [ "$JOBS" -le 16 ] || JOBS=16
units() { grep -v -e '^#' -e '^$' "$HERE/units.txt"; }
compile() { local unit="$1"; shift; $HIPCC $FLAGS "$@" -c "$HERE/$unit.hip" -o "$OBJ/${unit//\//_}.o"; }      # unit [its flags]
export -f compile
units | xargs -P "$JOBS" -L 1 bash -c 'compile "$@"' _
objs=(); while read -r unit _; do objs+=("$OBJ/${unit//\//_}.o"); done < <(units)
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/$NAME" "${objs[@]}"
echo "built $OUT/$NAME"
