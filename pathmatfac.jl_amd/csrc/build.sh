#!/bin/bash
# Builds libpmf_hip.so for gfx950 (hipcc cross-compiles without a GPU): csrc/Makefile, translation units in parallel.
# PMF_KEEP_TEMPS=dir keeps the device assembly (.s) of every unit there for inspection; that build runs one unit at a time,
# because the units compiled from one source file with different -D flags share the names of their temporaries and a parallel
# build lets them overwrite each other's device code.  Extra arguments go to hipcc.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
EXTRA="$*"
JOBS="${PMF_BUILD_JOBS:-8}"
if [[ -n "${PMF_KEEP_TEMPS:-}" ]]; then mkdir -p "$PMF_KEEP_TEMPS"; EXTRA="$EXTRA -save-temps=obj"; JOBS=1; fi
make -s -j"$JOBS" -C "$HERE" EXTRA="$EXTRA" ${PMF_LIB:+LIB="$PMF_LIB"} ${PMF_BUILD_DIR:+B="$PMF_BUILD_DIR"}
if [[ -n "${PMF_KEEP_TEMPS:-}" ]]; then
  bd="${PMF_BUILD_DIR:-.build}"; [[ "$bd" = /* ]] || bd="$HERE/$bd"   # (make -C: a relative build directory is relative to csrc)
  cp "$bd"/*.s "$PMF_KEEP_TEMPS"/ || echo "build.sh: no device assembly (.s) found in $bd" >&2
fi
