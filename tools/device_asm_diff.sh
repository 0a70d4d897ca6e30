#!/usr/bin/env bash
# Compare the device code of two source trees, translation unit by translation unit, without a GPU.
#
#   tools/device_asm_diff.sh OLD_TREE NEW_TREE [file.hip ...]
#
# For every .hip in the Makefile's SRC (or the ones named), with the Makefile's FLAGS, each tree is compiled with
# `--cuda-device-only -S` and the two assembly files are diffed.  The only line that differs between two compiles of
# the same code is the per-file `__hip_cuid_<hash>` symbol, which is filtered (see norm below).  A refactor that claims to leave the
# kernels alone must print "identical" for every unit.  Exit status: 0 when all are identical, 1 otherwise.
#
# The assembly is kept in $OUT (default: a fresh temporary directory) as old/<unit>.s and new/<unit>.s; an old/ that
# is already there is reused, so a long unit such as cgic_vq.hip is compiled once per baseline.  JOBS (default 8)
# compiles run at a time.
set -euo pipefail
[ $# -ge 2 ] || { echo "usage: $0 OLD_TREE NEW_TREE [file.hip ...]" >&2; exit 2; }
OLD=$(cd "$1" && pwd); NEW=$(cd "$2" && pwd); shift 2
OUT=${OUT:-$(mktemp -d)}
JOBS=${JOBS:-8}
CSRC=control-gic_amd/csrc

mkvar() {      # mkvar TREE NAME: the value of a Makefile variable, from the Makefile itself
    printf 'print-%%:\n\t@echo $($*)\n' | make -s --no-print-directory -C "$1/$CSRC" -f Makefile -f - "print-$2"
}
units() { if [ $# -gt 2 ]; then shift 2; echo "$@"; else mkvar "$1" SRC; fi; }

compile_tree() {      # compile_tree TREE SIDE units...
    local tree=$1 side=$2; shift 2
    local hipcc flags; hipcc=$(mkvar "$tree" HIPCC); flags=$(mkvar "$tree" FLAGS)
    mkdir -p "$OUT/$side"
    for u in "$@"; do
        [ "$side" = old ] && [ -s "$OUT/old/${u%.hip}.s" ] && continue
        [ -f "$tree/$CSRC/$u" ] || continue
        echo "$u"
    done | (cd "$tree/$CSRC" && xargs -r -P "$JOBS" -I{} sh -c \
        "$hipcc $flags -Wno-unused-command-line-argument --cuda-device-only -S {} -o '$OUT/$side/'\$(basename {} .hip).s") || echo "a compile failed in $tree (see above)" >&2
}

UNITS=$(units "$NEW" x "$@")
# shellcheck disable=SC2086
compile_tree "$OLD" old $UNITS
# shellcheck disable=SC2086
compile_tree "$NEW" new $UNITS

# what legitimately differs between two compiles of the same kernels: the per-file __hip_cuid_<hash> symbol, and the ordinal of a
# function inside its file in local labels (.LBB<fn>_<block>, .Lfunc_end<fn>), which shifts when a kernel before it was removed
norm() { sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g; s/\bL?BB[0-9]+_/BB_/g; s/\.Lfunc_(begin|end)[0-9]+/.Lfunc_\1/g' "$1"; }

status=0
for u in $UNITS; do
    s=${u%.hip}.s
    if [ ! -s "$OUT/old/$s" ] || [ ! -s "$OUT/new/$s" ]; then echo "$u: missing on one side"; status=1; continue; fi
    if d=$(diff <(norm "$OUT/old/$s") <(norm "$OUT/new/$s")); then
        echo "$u: identical ($(wc -l < "$OUT/new/$s") lines)"
    else
        status=1
        echo "$u: DIFFERS ($(grep -c '^[<>]' <<<"$d") lines).  Kernels on one side only, then every hunk with its first line:"
        grep -E '^[<>][[:space:]]*\.amdhsa_kernel ' <<<"$d" | sed 's/^/    /' || true
        awk '/^[0-9]/ { h = $0; getline; print "    " h ": " $0 }' <<<"$d" | awk 'NR <= 40'
    fi
done
echo "assembly kept in $OUT"
exit $status
