#!/bin/bash
# build_full_variant.sh TAG [hipcc flags...]: libsfx_TAG.so with EVERY unit of csrc/units.txt compiled under the extra flags
set -e
CSRC="$(cd "$(dirname "${BASH_SOURCE[0]}")/../smplify-x-partial_amd/csrc" && pwd)"; TAG=$1; shift
SFX_NAME="libsfx_$TAG.so" SFX_OBJ="${TMPDIR:-/tmp}/v_$TAG" SFX_DEFINES="$SFX_DEFINES $*" bash "$CSRC/build.sh"
