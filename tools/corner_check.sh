#!/usr/bin/env bash
# Host build + run of tools/corner_check.hip (no GPU needed).  usage: tools/corner_check.sh INPUT [INPUT ...]
# The library's floating-point flags, so that host and device round alike.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="${TMPDIR:-/tmp}/corner_check"
/opt/rocm/bin/hipcc -O2 -std=c++17 -ffp-contract=off --offload-arch=gfx950 ${CORNER_CHECK_CXXFLAGS:-} \
  -I"$here/../include" "$here/corner_check.hip" -o "$out"
"$out" "$@"
