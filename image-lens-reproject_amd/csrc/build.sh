#!/usr/bin/env bash
# Builds liblrp_hip.so (gfx950) in-tree.  Usage: build.sh [jobs]
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${LRP_BUILD_OUT:-$here/../lib}"   # (LRP_BUILD_OUT / LRP_BUILD_FLAGS: variant builds for same-box A/B timing, tools/ablate.sh)
obj="$out/obj"
mkdir -p "$out" "$obj"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# Compilers at once: the argument, else $MAX_JOBS, else $CMAKE_BUILD_PARALLEL_LEVEL, else min(nproc, 16) — nproc counts the whole
# machine, of which a container or a batch slot may use a part, and a window-kernel unit takes 1-2 GiB.
cpus="$(nproc)"
jobs="${1:-${MAX_JOBS:-${CMAKE_BUILD_PARALLEL_LEVEL:-$(( cpus < 16 ? cpus : 16 ))}}}"
# Parity flags: no FMA contraction, IEEE divide/sqrt, denormals kept, no fast-math.  --offload-compress: the code objects are
# stored compressed in the fat binary (the runtime unpacks them when the library is loaded): liblrp_hip.so 39.7 -> ~8 MB.
FLAGS=(--offload-arch=gfx950 --offload-compress -std=c++17 -O3 -fPIC -ffp-contract=off
       -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-gpu-flush-denormals-to-zero
       -Wall -Wno-unused-function -Wno-inline-asm -Wno-cuda-compat -I"$here" -I"$here/../../include" ${LRP_BUILD_FLAGS:-})
# The objects, in link order: units.list, a line each — object, source, that unit's -D defines and code generation options.
list="$here/units.list"
objs=(); srcs=(); opts=()
while read -r o s rest; do
  [[ -z "$o" || "$o" == \#* ]] && continue
  objs+=("$obj/$o"); srcs+=("$here/$s"); opts+=("$rest")
done < "$list"
pids=()
for i in "${!objs[@]}"; do
  o="${objs[$i]}"; s="${srcs[$i]}"
  if [[ ! -f "$o" || "$s" -nt "$o" || -n "$(find "$here" -maxdepth 1 -name '*.h' -newer "$o" -print -quit)" \
        || "$here/../../include/lrp.h" -nt "$o" || "${BASH_SOURCE[0]}" -nt "$o" || "$list" -nt "$o" ]]; then
    # at most $jobs compilers at once (a window-kernel unit takes 1-2 GiB)
    while (( $(jobs -rp | wc -l) >= jobs )); do wait -n || true; done
    # shellcheck disable=SC2086
    ( "$HIPCC" "${FLAGS[@]}" ${opts[$i]} -x hip -c "$s" -o "$o" ) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [[ -n "$p" ]] && wait "$p"; done
for o in "$obj"/*.o; do [[ " ${objs[*]} " == *" $o "* ]] || rm -f "$o"; done # (an object the manifest no longer names)
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o "$out/liblrp_hip.so" "${objs[@]}"
echo "built $out/liblrp_hip.so"
