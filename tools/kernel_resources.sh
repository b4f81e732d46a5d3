#!/usr/bin/env bash
# VGPR / SGPR / spill counts of every kernel of the given units (device-only assembly; no GPU needed).
# usage: tools/kernel_resources.sh lrp_tile_winq [more units] [-- extra hipcc flags]
# A unit is an object of csrc/units.list, with or without ".o"; it is compiled from the manifest's source with the manifest's
# -D defines; the unit's other options (units.list) only when given after "--".
set -euo pipefail
root="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
src="$root/image-lens-reproject_amd/csrc"
units=(); extra=()
while [[ $# -gt 0 ]]; do if [[ "$1" == "--" ]]; then shift; extra=("$@"); break; fi; units+=("${1%.o}"); shift; done
tmp="$(mktemp -d)"
for u in "${units[@]}"; do
  line="$(awk -v o="$u.o" '$1 == o' "$src/units.list")"
  [[ -n "$line" ]] || { echo "not in csrc/units.list: $u" >&2; exit 2; }
  read -r _ s rest <<< "$line"
  defs=(); for w in $rest; do [[ "$w" == -D* ]] && defs+=("$w"); done
  ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt \
      -fno-fast-math -fno-gpu-flush-denormals-to-zero -I"$src" -I"$root/include" "${defs[@]}" "${extra[@]}" -x hip -c "$src/$s" \
      --cuda-device-only -S -o "$tmp/$u.s" 2>/dev/null ) &
done
wait
for u in "${units[@]}"; do
  echo "== $u"
  grep -E "^\s+\.name:|\.vgpr_count|\.vgpr_spill_count|\.sgpr_spill_count|\.sgpr_count" "$tmp/$u.s" | paste - - - - - |
    sed -E 's/\s+/ /g; s/_ZN3lrp[0-9]+//; s/EEvNS_7KParamsE//' |
    awk '{printf "%-60s sgpr %s (spilled %s) vgpr %s (spilled %s)\n", $2, $4, $6, $8, $10}'
done
if [[ -n "${KEEP_ASM:-}" ]]; then echo "assembly kept in $tmp"; else rm -rf "$tmp"; fi
