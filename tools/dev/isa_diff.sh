#!/bin/bash
# usage: tools/dev/isa_diff.sh <parent-tree> <file.hip>   — compiles one source of tokengeex_amd/csrc from another checkout
# of the repository (the parent commit, say) and from this one for gfx950, with the library's flags, and diffs the
# instruction streams: comment and directive lines dropped, labels and instructions kept.  Prints the diff and exits 0
# when the streams are identical, 1 when they are not.
set -e
set -o pipefail
PARENT=$(cd "$1" && pwd); SRC=$2
HERE=$(cd "$(dirname "$0")/../.." && pwd)
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
for side in parent new; do
    if [ $side = parent ]; then CS=$PARENT/tokengeex_amd/csrc; else CS=$HERE/tokengeex_amd/csrc; fi
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -munsafe-fp-atomics -Wall -Wno-unused-result -Wno-pass-failed \
        -x hip -S "$CS/$SRC" -o "$OUT/$side.s" --cuda-device-only
    # keep labels and instructions: no blank lines, no comment lines, no directives, no trailing comments, and not the
    # compilation unit's id symbol, which is a hash of the source text
    sed -e 's/[[:space:]]*;.*$//' "$OUT/$side.s" | grep -v -e '^[[:space:]]*$' -e '^[[:space:]]*\.' -e '^__hip_cuid_' > "$OUT/$side.isa"
done
echo "$SRC: $(wc -l < "$OUT/parent.isa") lines in the parent's stream, $(wc -l < "$OUT/new.isa") in this tree's"
if diff "$OUT/parent.isa" "$OUT/new.isa"; then echo "$SRC: identical"; else echo "$SRC: DIFFERENT"; exit 1; fi
