#!/usr/bin/env bash
# Device-only assembly of every translation unit of a tree's drtvam_amd/csrc (build.sh's flags plus
# --cuda-device-only -S; no GPU needed), one line per file: sha256, line count, file name.  Two
# trees whose lines agree run the same device code.
# usage: tools/device_asm_hashes.sh [TREE]   (default: this tree)
set -euo pipefail
tree="$(cd "${1:-$(dirname "$0")/..}" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
tmp="$(mktemp -d "${TMPDIR:-/tmp}/tvam_asm.XXXXXX")"
trap 'rm -rf "$tmp"' EXIT
flags=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC
       -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -munsafe-fp-atomics
       -Wall -Wno-unused-function -I"$tree/include" --cuda-device-only -S -fuse-cuid=none)
cd "$tree/drtvam_amd/csrc"
pids=()
for src in *.hip; do
  "$HIPCC" "${flags[@]}" "$src" -o "$tmp/${src%.hip}.s" &
  pids+=($!)
done
for pid in "${pids[@]}"; do wait "$pid"; done
for src in *.hip; do
  s="$tmp/${src%.hip}.s"
  printf '%s %6d %s\n' "$(sha256sum < "$s" | cut -d' ' -f1)" "$(wc -l < "$s")" "$src"
done
