#!/bin/bash
# Product device code before/after a source refactor that must leave the kernels as they are: the gfx950
# assembly of one translation unit with the product flags, comments and debug directives stripped, compared with a saved copy.  Only the
# per-compilation __hip_cuid_* symbol may differ.  Runs on the build host (no GPU).  An optional fourth argument
# holds extra compile flags, so the A/B build can be compared too.
#   scripts/product_isa_equal.sh save tower.hip /tmp/base.s     (before)
#   scripts/product_isa_equal.sh cmp  tower.hip /tmp/base.s     (after)
#   scripts/product_isa_equal.sh save tower.hip /tmp/base_ab.s -DSPMCTS_AB
# cmp first compares the files as they are; if they differ it compares per kernel symbol: each symbol's text
# section (instructions, .amdhsa_kernel descriptor, register counts) together with its entry of the metadata
# section (LDS, scratch, spills, arguments), with the function index of local labels (.LBB<n>_<m>,
# .Lfunc_end<n>) dropped, so the order in which the host code instantiates the kernels does not count.  It
# reports the symbols only one side has and, per differing symbol, how many lines differ.
#   scripts/product_isa_equal.sh symbols tower.hip /tmp/base.s  (the saved copy's symbols, no compile)
#   scripts/product_isa_equal.sh cmp /tmp/new.s /tmp/base.s      (two saved copies, absolute paths, no compile)
set -e
set -o pipefail
mode=$1; src=$2; ref=$3; extra=$4
cd "$(dirname "$0")/../self_play_reinforcement_learning_amd/csrc"

# stdin: stripped assembly; stdout: "symbol<TAB>line", sorted by symbol (a symbol's lines keep their order)
by_symbol() {
  sed 's/\.L\([A-Za-z_]*[A-Za-z_]\)[0-9][0-9]*/.L\1/g' | awk '
    function flush(   i) { for (i = 0; i < n; ++i) print name "\t" ent[i]; n = 0; name = "(metadata)" }
    BEGIN { key = "(module)"; name = "(metadata)" }
    meta && /^  - \./ { flush() }
    meta && /^[^ ]/ { flush(); meta = 0; key = "(module)" }
    meta { ent[n++] = $0; if ($1 == ".name:") name = $2; next }
    /^amdhsa\.kernels:/ { print "(module)\t" $0; meta = 1; next }
    /^\t\.section\t\.text\./ { key = $2; sub(/^\.text\./, "", key); sub(/,.*/, "", key) }
    /^\t\.section\t\.AMDGPU\.gpr_maximums/ { key = "(module)" }
    { print key "\t" $0 }' | LC_ALL=C sort -s -t"$(printf '\t')" -k1,1
}
symbols() { cut -f1 "$1" | uniq | grep -v '^(m'; }

if [ "$mode" = symbols ]; then by_symbol < "$ref" > "$ref.sym"; symbols "$ref.sym"; rm -f "$ref.sym"; exit 0; fi
out=$(mktemp)
if [ "${src%.s}" != "$src" ]; then
  cp "$src" "$out"  # a copy saved earlier instead of a source file: cmp of two saved copies
else
  /opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fno-gpu-rdc -I../../include $extra \
    --offload-device-only -S "$src" -o "$out.raw" 2>/dev/null
  grep -v '^\s*;' "$out.raw" | sed 's/\s*;.*$//' | grep -v '^\s*\.\(file\|loc\|ident\)' | grep -v 'amdhsa.version\|\.amdgcn_target\|^\s*$' \
    | grep -v '__hip_cuid_' > "$out"
  rm -f "$out.raw"
fi
if [ "$mode" = save ]; then mv "$out" "$ref"; echo "saved $(wc -l < "$ref") lines, $(grep -c s_endpgm "$ref") kernels"; exit 0; fi
if cmp -s "$out" "$ref"; then
  echo "identical: $(wc -l < "$ref") lines, $(grep -c s_endpgm "$ref") kernels, $(grep -c '^\s*\.amdhsa_kernel ' "$ref") kernel symbols"
  rm -f "$out"; exit 0
fi
by_symbol < "$ref" > "$out.a"; by_symbol < "$out" > "$out.b"
symbols "$out.a" > "$out.sa"; symbols "$out.b" > "$out.sb"
trap 'rm -f "$out" "$out.a" "$out.b" "$out.sa" "$out.sb"' EXIT
rc=0
if cmp -s "$out.sa" "$out.sb"; then
  echo "symbol sets equal: $(wc -l < "$out.sa") symbols"
else
  rc=1; echo "symbol sets differ (< saved only, > now only):"; diff "$out.sa" "$out.sb" | grep '^[<>]' || true
fi
if cmp -s "$out.a" "$out.b"; then
  echo "identical per symbol (other order): $(wc -l < "$ref") lines, $(grep -c s_endpgm "$ref") kernels"
else
  rc=1; echo "differing lines per symbol:"
  (diff "$out.a" "$out.b" || true) | grep '^[<>]' | cut -c3- | cut -f1 | LC_ALL=C sort | uniq -c
  (diff "$out.a" "$out.b" || true) | cut -f2- | head -20
fi
exit $rc
