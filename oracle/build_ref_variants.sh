#!/usr/bin/env bash
# Compile variants of the reference solvers at other grids and geometries.
# The reference programs take no command line: grid, physics and run length
# are named constants in their solver classes. For each variant below the
# reference source is streamed through sed, which replaces the VALUE of the
# named constants, straight into the compiler's standard input. Only binaries
# are written, under oracle/_ref/variants/ (git-ignored); no substituted
# source is stored anywhere. This recipe holds constant names and new values,
# nothing else of the reference.
#
# Every substitution must match exactly one line of the source, or the script
# fails. (tests/golden/make_ref_variants.py additionally asserts that each
# binary's own "Grid:" line shows the intended size.)
#
# Usage: oracle/build_ref_variants.sh [REF_DIR]   (default /root/reference)
#        oracle/build_ref_variants.sh --list      (print the table, build nothing)
set -euo pipefail

# name | case | NAME=value ...
# Every run is short (final_time) and prints and saves every step, so each
# Step line and the last frame are recorded.
# Cavity: dt = 0.5*min(0.25 h^2 Re, h), h = 1/n: the convective limit holds
# for h > 4/Re (n=2, 3, 20 at Re 1000), the diffusive one for n=20 at Re 10
# and n=16 at Re 40.
# Step: dx = 8/NX, dy = 2/NY; step_i = (int)(STEP_LOCATION/dx), inlet_jmax =
# (int)(HEIGHT_INLET/dy). 12x6 and 60x12 have a dx that is no binary fraction
# (2/dx = 3 and 15 only if the division rounds that way); 448x8 puts step_i on
# 112; 64x32 at 0.2 gives step_i = 1; 40x10 at 1.9 gives inlet_jmax = ny-1;
# 4x2 gives both at once.
VARIANTS='
cavity_n2|cavity|n_interior=2 final_time=1.0 print_interval=1 save_data_interval=1
cavity_n3|cavity|n_interior=3 final_time=0.7 print_interval=1 save_data_interval=1
cavity_n20|cavity|n_interior=20 final_time=0.1 print_interval=1 save_data_interval=1
cavity_n20_re10|cavity|n_interior=20 reynolds_number=10.0 final_time=0.02 print_interval=1 save_data_interval=1
cavity_n16_re40|cavity|n_interior=16 reynolds_number=40.0 final_time=0.08 print_interval=1 save_data_interval=1
channel_2x2|channel|NX_INT=2 NY_INT=2 final_time=0.5 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
channel_3x2|channel|NX_INT=3 NY_INT=2 final_time=0.4 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
channel_2x7|channel|NX_INT=2 NY_INT=7 final_time=0.12 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
channel_13x5|channel|NX_INT=13 NY_INT=5 final_time=0.15 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
channel_17x40|channel|NX_INT=17 NY_INT=40 final_time=0.012 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
channel_50x17|channel|NX_INT=50 NY_INT=17 final_time=0.05 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_4x2|backwards_step|NX_INT=4 NY_INT=2 final_time=0.7 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_5x3|backwards_step|NX_INT=5 NY_INT=3 final_time=0.4 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_9x2|backwards_step|NX_INT=9 NY_INT=2 final_time=0.6 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_12x6|backwards_step|NX_INT=12 NY_INT=6 final_time=0.2 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_60x12|backwards_step|NX_INT=60 NY_INT=12 final_time=0.09 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_100x20|backwards_step|NX_INT=100 NY_INT=20 final_time=0.05 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_448x8|backwards_step|NX_INT=448 NY_INT=8 final_time=0.0035 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_64x32_i1|backwards_step|NX_INT=64 NY_INT=32 STEP_LOCATION=0.2 final_time=0.04 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
step_40x10_j9|backwards_step|NX_INT=40 NY_INT=10 HEIGHT_INLET=1.9 final_time=0.13 PRINT_INTERVAL=1 SAVE_DATA_INTERVAL=1
'

if [ "${1:-}" = "--list" ]; then
  printf '%s' "$VARIANTS" | grep -v '^$'
  exit 0
fi

REF="${1:-/root/reference}"
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/_ref/variants"
if [ ! -d "$REF" ]; then
  echo "reference tree $REF not present; skipping reference variants" >&2
  exit 0
fi
mkdir -p "$OUT"

printf '%s' "$VARIANTS" | grep -v '^$' | while IFS='|' read -r name case subs; do
  src="$REF/$case-01.cpp"
  bin="$OUT/$name"
  if [ -x "$bin" ] && [ "$bin" -nt "$src" ] && [ "$bin" -nt "$0" ]; then
    continue
  fi
  prog=()
  for kv in $subs; do
    key="${kv%%=*}"; val="${kv#*=}"
    # the declaration "static constexpr <type> KEY = <value>;" of the solver class
    decl="^[[:space:]]*static constexpr [a-z]+[[:space:]]+${key}[[:space:]]*="
    n="$(grep -Ec "$decl" "$src" || true)"
    if [ "$n" != "1" ]; then
      echo "variant $name: constant $key matches $n lines of $src, expected exactly 1" >&2
      exit 1
    fi
    prog+=(-e "s/(${decl}[[:space:]]*)[^;]*;/\\1${val};/")
  done
  sed -E "${prog[@]}" "$src" | g++ -std=c++17 -O2 -w -x c++ - -o "$bin"
done
echo "built reference variants into $OUT"
