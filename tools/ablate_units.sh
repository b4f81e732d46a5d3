#!/usr/bin/env bash
# Variant of liblrp_hip.so for same-box A/B timing in which only SOME units are recompiled with other options:
#   tools/ablate_units.sh <name> "<unit> ..." [hipcc options ...]
# A unit is an object of csrc/units.list, with or without ".o" (lrp_tile_wing, lrp_camgain_bc.o).  Builds
# tools/_ablate/<name>/liblrp_hip.so from those units (compiled here from the manifest's source with the manifest's -D
# defines, WITHOUT the unit's other options unless given) and the up-to-date objects of image-lens-reproject_amd/lib/obj.
# Run with
#   LD_LIBRARY_PATH=tools/_ablate/<name> tools/kbench ...
set -euo pipefail
root="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
src="$root/image-lens-reproject_amd/csrc"; obj="$root/image-lens-reproject_amd/lib/obj"
name="$1"; units="$2"; shift 2
out="$root/tools/_ablate/$name"; rm -rf "$out"; mkdir -p "$out"
FLAGS=(--offload-arch=gfx950 -std=c++17 -O3 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
       -fno-fast-math -fno-gpu-flush-denormals-to-zero -Wno-unused-function -Wno-inline-asm -I"$src" -I"$root/include" "$@")
pids=(); objs=(); left=" $units "
while read -r o s rest; do
  [[ -z "$o" || "$o" == \#* ]] && continue
  if [[ "$left" == *" $o "* || "$left" == *" ${o%.o} "* ]]; then
    left="${left/ $o / }"; left="${left/ ${o%.o} / }"
    defs=(); for w in $rest; do [[ "$w" == -D* ]] && defs+=("$w"); done
    ( /opt/rocm/bin/hipcc "${FLAGS[@]}" "${defs[@]}" -x hip -c "$src/$s" -o "$out/$o" ) & pids+=($!)
    objs+=("$out/$o")
  else
    objs+=("$obj/$o")
  fi
done < "$src/units.list"
[[ -z "${left// /}" ]] || { echo "not in csrc/units.list:$left" >&2; exit 2; }
for p in "${pids[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/liblrp_hip.so" "${objs[@]}"
rm -f "$out"/*.o
echo "built $out/liblrp_hip.so"
