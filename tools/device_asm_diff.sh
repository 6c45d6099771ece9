#!/bin/bash
# Device assembly of every .hip source, this tree against another (compile-only, host side): the check a refactor
# that must not change the generated code rests on.
# usage: tools/device_asm_diff.sh <other-tree>   (a checkout of the commit to compare with; run from the repository root)
# Each source is compiled in both trees with the flags of cattleherd/_build.py (FLAGS, and SOURCE_FLAGS for the sources
# that have them) plus --cuda-device-only -S.  The only difference allowed is the compilation-unit id symbol
# (__hip_cuid_<hash>, a hash of the source path and text); everything else -- kernel bodies, .amdhsa_* directives,
# kernel order, metadata -- must be byte-equal.  Prints one line per source and exits 1 if any differs.
# KEEP=dir keeps the .s files there (default: a temporary directory, removed at the end) and reuses the other tree's
# files found there, so repeated runs during a refactor compile only this tree.
set -u
OTHER=${1:?usage: tools/device_asm_diff.sh <other-tree>}
PKG=rl-cattle-herding_amd
OUT=${KEEP:-$(mktemp -d)}
mkdir -p "$OUT/this" "$OUT/other"

# "<source> <flags...>" per .hip source, from the build script of the tree at $1
cmds() {
  (cd "$1/$PKG/cattleherd" && python3 -B -c '
import _build as b
for s in b.SOURCES:
    if s.endswith(".hip"):
        print(s, *[f for f in b.FLAGS if not f.startswith("-I")], *b.SOURCE_FLAGS.get(s, []))')
}
asm() {   # tree, side
  cmds "$1" | while read -r src flags; do
    [ "$2" = other ] && [ -s "$OUT/other/$src.s" ] && continue
    echo "cd '$1' && ${HIPCC:-/opt/rocm/bin/hipcc} $flags -Iinclude --cuda-device-only -S $PKG/csrc/$src -o '$OUT/$2/$src.s' 2>'$OUT/$2/$src.log'"
  done
}
rm -f "$OUT"/this/*.s
{ asm "$(cd "$OTHER" && pwd)" other; asm "$(pwd)" this; } | xargs -P "${JOBS:-8}" -I{} sh -c {}

rc=0
for f in $(cmds "$(pwd)" | cut -d' ' -f1); do
  s="$OUT/this/$f.s"
  if [ ! -s "$s" ] || [ ! -s "$OUT/other/$f.s" ]; then
    echo "$f: did not compile in both trees"; cat "$OUT/this/$f.log" "$OUT/other/$f.log" 2>/dev/null | tail -5; rc=1; continue
  fi
  if cmp -s <(sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$s") <(sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$OUT/other/$f.s"); then
    echo "$f: identical but for the unit id ($(grep -c '^\s*\.amdhsa_kernel ' "$s") kernels, $(wc -l < "$s") lines)"
  else
    echo "$f: DIFFERS"; rc=1
    # which of its kernels do: a change may edit some instantiations of a file and must leave the others alone
    python3 -B "$(dirname "$0")/device_asm_kernels.py" "$s" "$OUT/other/$f.s" | sed 's/^/    /'
  fi
done
[ -n "${KEEP:-}" ] || rm -rf "$OUT"
exit $rc
