#!/bin/bash
# Check that a source-only change leaves the emitted device code alone:
#     tools/device_asm_diff.sh <rev-a> <rev-b> [workdir]
# exports both revisions with `git archive` into <workdir>/a and <workdir>/b (default: a fresh temporary directory),
# compiles every csrc/*.hip of each, from the same relative directory, with the flags of _lib.build() plus
# `--cuda-device-only -S` (gfx950 assembly; cross-compiles without a GPU, at most 16 jobs) and diffs the assembly files
# pairwise, .amdgpu_metadata (VGPR / AGPR / SGPR counts, LDS and scratch bytes) included.  Nothing is filtered: any
# differing line counts.  <rev-b> may be WORKTREE for the uncommitted working tree.  Exit status 0 iff the two
# revisions have the same units and every pair is identical.
set -eu
A=$1; B=$2
cd "$(dirname "$0")/.."
WORK=${3:-$(mktemp -d)}
PKG=behavior_driven_video_synthesis_amd
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result --cuda-device-only -S"

compile_rev() {  # <rev> <dir>: export csrc/ and include/ (nothing else is read by the compile) and compile every unit
    local id; [ "$1" = WORKTREE ] && id=WORKTREE || id=$(git rev-parse "$1^{commit}")
    # a committed revision already compiled in a reused <workdir> is not compiled again
    [ "$id" != WORKTREE ] && [ "$(cat "$2/rev" 2>/dev/null)" = "$id" ] && return 0
    rm -rf "$2"; mkdir -p "$2/$PKG" "$2/asm"
    if [ "$id" = WORKTREE ]; then cp -r $PKG/csrc "$2/$PKG/csrc"; cp -r include "$2/include"
    else git archive "$id" $PKG/csrc include | tar -x -C "$2"; fi
    # relative paths only, so no directive can name the scratch directory
    (cd "$2" && ls $PKG/csrc/*.hip | xargs -P "${JOBS:-16}" -I{} sh -c \
        "$HIPCC $FLAGS {} -o asm/\$(basename {} .hip).s || { echo 'hipcc failed on {}' >&2; exit 255; }")
    echo "$id" > "$2/rev"
}

compile_rev "$A" "$WORK/a"; compile_rev "$B" "$WORK/b"

n=0; same=0; differing=""
for u in $( (cd "$WORK/a/asm" && ls *.s; cd "$WORK/b/asm" && ls *.s) | sort -u ); do
    n=$((n + 1))
    if [ -f "$WORK/a/asm/$u" ] && [ -f "$WORK/b/asm/$u" ] && cmp -s "$WORK/a/asm/$u" "$WORK/b/asm/$u"; then same=$((same + 1))
    else differing="$differing ${u%.s}"; fi
done
echo "$A vs $B: $same of $n units identical (assembly in $WORK)"
for u in $differing; do
    echo "DIFFERS: $u  ($( (diff "$WORK/a/asm/$u.s" "$WORK/b/asm/$u.s" 2>&1 || true) | grep -c '^[<>]') lines)"
done
[ -z "$differing" ]
