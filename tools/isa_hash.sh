#!/usr/bin/env bash
# sha256 of the gfx950 machine code of every kernel object in a directory (one line per object): two builds whose sources differ
# only in dead alternatives print the same lines.  usage: isa_hash.sh <obj-dir>
# Per kernel (tools/isa_kernels.py: a position-independent hash and the resource line of every kernel symbol, so that a kernel
# may move between objects):  isa_hash.sh --kernels <obj-dir>  |  isa_hash.sh --compare <obj-dir-a> <obj-dir-b>
set -euo pipefail
case "${1:-}" in
  --kernels|--compare) mode="${1#--}"; shift; exec python3 "$(dirname "${BASH_SOURCE[0]}")/isa_kernels.py" "$mode" "$@" ;;
esac
B=/opt/rocm/lib/llvm/bin
tmp=$(mktemp -d); trap 'rm -rf $tmp' EXIT
for o in "$1"/*.o; do
  n=$(basename "$o")
  if $B/llvm-objcopy --dump-section .hip_fatbin=$tmp/fat.bin "$o" /dev/null 2>/dev/null && [ -s $tmp/fat.bin ]; then
    $B/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/fat.bin --output=$tmp/dev.co --unbundle 2>/dev/null
    echo "$n $($B/llvm-objdump -d $tmp/dev.co | grep -v "file format" | sha256sum | cut -c1-16)"
  else
    echo "$n host-only $(sha256sum < "$o" | cut -c1-16)"
  fi
  rm -f $tmp/fat.bin $tmp/dev.co
done
