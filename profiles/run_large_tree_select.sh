#!/bin/bash
# Selection / preplacement / lookup / Newton kernel times on large references, the change against its parent:
#   bash profiles/run_large_tree_select.sh PARENT_ROOT [OUT_DIR]
# PARENT_ROOT: a directory holding the parent commit's built epa_ng_amd/ package (git archive + build.py).
# Child processes alternate between the two packages; every GPU step has its own time limit and the chain
# stops at the first failure.  Output: OUT_DIR/large_tree_select.jsonl (one JSON line per case).
set -u
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$HERE")"
PARENT="${1:?parent package root}"
OUT="${2:-${EPA_PROF_OUT:-prof_out}}"
mkdir -p "$OUT"
J="$OUT/large_tree_select.jsonl"
: > "$J"
run() {   # tag, package root, further arguments
  local tag="$1" root="$2"; shift 2
  timeout -k 10 240 python "$HERE/large_tree_select.py" --pkg-root "$root" --tag "$tag" "$@" >> "$J" 2>> "$OUT/large_tree_select.err"
}
run parent "$PARENT" --tips 32769 &&
run branch "$ROOT" --tips 32769 &&
run parent "$PARENT" --tips 32769 &&
run branch "$ROOT" --tips 32769 &&
run branch "$ROOT" --tips 32770 &&
run branch "$ROOT" --tips 32770 --flat &&
run parent "$PARENT" --tips 8194 --width 96 --read-len 64 &&
run branch "$ROOT" --tips 8194 --width 96 --read-len 64
rc=$?
cat "$J"
tail -5 "$OUT/large_tree_select.err" 2>/dev/null
exit $rc
