#!/bin/bash
# development: compare the gfx950 device code of this tree's HIP units with another tree's (a checkout of the parent commit), for a
# refactor that must leave every kernel as it was.
# usage: tools/unit_isa_diff.sh PARENT_TREE [unit ...]      (unit = gemv_q4k, gemm_lw, ...; default: every unit in the Makefile's HIP_SRCS)
# Builds UNIT.o in both trees with csrc/Makefile's own rules (so the per-unit flags are the product's; an object that is up to date
# is not rebuilt), takes the gfx950 code object out of each (llvm-objdump --offloading), disassembles it (llvm-objdump -d) and
# prints per unit `same` or the number of differing disassembly lines.  A unit without device code says so.  Exit status 1 on any
# difference.  At most 16 build jobs (JOBS=n for fewer).  KEEP=dir keeps the disassemblies (dir/{here,parent}/UNIT.s).
set -e -o pipefail
[ $# -ge 1 ] || { sed -n '2,8p' "$0"; exit 2; }
HERE=$(cd "$(dirname "$0")/.." && pwd)
PARENT=$(cd "$1" && pwd)
shift
CS=llamafile_amd/csrc
OBJDUMP=${OBJDUMP:-/opt/rocm/llvm/bin/llvm-objdump}
UNITS=${*:-$(sed -n 's/^HIP_SRCS = //p' "$HERE/$CS/Makefile" | sed 's/\.hip//g')}
JOBS=${JOBS:-$(nproc)}
[ "$JOBS" -le 16 ] || JOBS=16
OUT=${KEEP:-$(mktemp -d)}
[ -n "$KEEP" ] || trap 'rm -rf "$OUT"' EXIT

objs=""
for u in $UNITS; do objs="$objs $u.o"; done
for tree in "$HERE" "$PARENT"; do
    make -s -C "$tree/$CS" -j"$JOBS" $objs
done

# the disassembly of UNIT's gfx950 code object in tree $1 -> $2/UNIT.s (empty: no device code)
disasm() {
    local tree=$1 dst=$2 u=$3
    mkdir -p "$dst/x_$u"
    cp "$tree/$CS/$u.o" "$dst/x_$u/$u.o"
    (cd "$dst/x_$u" && "$OBJDUMP" --offloading "$u.o" > /dev/null)
    : > "$dst/$u.s"
    for co in "$dst/x_$u"/*gfx950*; do
        [ -e "$co" ] || continue
        "$OBJDUMP" -d "$co" | grep -v 'file format' >> "$dst/$u.s"
    done
    rm -rf "$dst/x_$u"
}

bad=0
for u in $UNITS; do
    disasm "$HERE" "$OUT/here" "$u"
    disasm "$PARENT" "$OUT/parent" "$u"
    if [ ! -s "$OUT/here/$u.s" ] && [ ! -s "$OUT/parent/$u.s" ]; then
        echo "$u: same (no device code)"
    elif cmp -s "$OUT/here/$u.s" "$OUT/parent/$u.s"; then
        echo "$u: same ($(grep -c . "$OUT/here/$u.s") lines)"
    else
        # (counted on the instruction text alone: with the address and encoding beside it, one inserted instruction would count
        # every line behind it)
        n=$(diff <(sed 's_ *//.*__' "$OUT/parent/$u.s") <(sed 's_ *//.*__' "$OUT/here/$u.s") | grep -c '^[<>]' || true)
        echo "$u: $n instruction lines differ (of $(grep -c . "$OUT/parent/$u.s") / $(grep -c . "$OUT/here/$u.s"))"
        bad=1
    fi
done
exit $bad
