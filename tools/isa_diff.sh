#!/bin/bash
# Instruction check of a refactor: the gfx950 code of csrc/<unit>.hip in two trees, kernel by kernel.  Needs no GPU.
#   git worktree add /tmp/parent HEAD~1 && bash tools/isa_diff.sh /tmp/parent . nr_topk nr_rank nr_logz nr_mmr nr_data
# Per kernel symbol: `same`, or the instruction counts in A and B; then the diff of the symbol lists and of the descriptor
# fields (registers, LDS, scratch, kernarg size) of the code object's notes.  Whole-text diffs of the disassembly without
# addresses and encodings (the code objects themselves differ: HIP embeds a per-file id).  Exit status 1 if anything differs.
set -euo pipefail
A=$1; B=$2; shift 2
ROCM=${ROCM_PATH:-/opt/rocm}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-variable -ffp-contract=fast --offload-device-only"
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
status=0
units=("$@"); [ ${#units[@]} -gt 0 ] || units=(nr_topk nr_rank nr_logz nr_mmr nr_data)
for u in "${units[@]}"; do
  for t in A B; do
    mkdir -p "$T/$t.$u"
    "$ROCM/bin/hipcc" $FLAGS -c "${!t}/newsrecommendation_amd/csrc/$u.hip" -o "$T/$t.$u.o"
    "$ROCM/llvm/bin/clang-offload-bundler" --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input="$T/$t.$u.o" --output="$T/$t.$u.co"
    # one file of instructions per symbol; "..." is the zero padding behind a function, which depends on its neighbours
    "$ROCM/llvm/bin/llvm-objdump" -d --no-show-raw-insn --no-leading-addr "$T/$t.$u.co" | sed 's@ *//.*@@' |
      awk -v d="$T/$t.$u" '/^<.*>:$/ { f = d "/" substr($0, 2, length($0) - 3); next } f != "" && NF && $1 != "..." { print > f }'
    ls "$T/$t.$u" > "$T/$t.$u.syms"
    "$ROCM/llvm/bin/llvm-readelf" --notes "$T/$t.$u.co" | awk '
      /^  - \.agpr_count:/ { r = " agpr_count:" $3 }
      /^    \.(group_segment_fixed_size|kernarg_segment_size|private_segment_fixed_size|sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count):/ { r = r " " substr($1, 2) $2 }
      /^    \.name:/ { n = $2 }
      /^    \.wavefront_size:/ { print n r }' | sort > "$T/$t.$u.desc"
  done
  echo "== $u"
  same=0; differ=0
  for k in $(comm -12 "$T/A.$u.syms" "$T/B.$u.syms"); do
    if cmp -s "$T/A.$u/$k" "$T/B.$u/$k"; then same=$((same + 1)); [ -n "${VERBOSE:-}" ] && echo "same $k"
    else differ=$((differ + 1)); echo "$(wc -l < "$T/A.$u/$k") -> $(wc -l < "$T/B.$u/$k") instructions  $k"; fi
  done
  echo "$same kernels same, $differ differ"
  diff "$T/A.$u.syms" "$T/B.$u.syms" > "$T/d" && echo "symbol lists identical" || { echo "symbol lists differ:"; cat "$T/d"; status=1; }
  diff "$T/A.$u.desc" "$T/B.$u.desc" > "$T/d" && echo "descriptor fields identical" || { echo "descriptor fields differ:"; cat "$T/d"; status=1; }
  [ "$differ" -eq 0 ] || status=1
done
exit $status
