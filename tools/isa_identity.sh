#!/bin/bash
# Is the gfx950 device assembly of every esvit_amd/csrc/*.hip the same as in another tree (the parent commit, say)?
#   mkdir /tmp/parent && git archive HEAD | tar -x -C /tmp/parent && bash tools/isa_identity.sh /tmp/parent [workdir [stem ...]]
# Compiles each translation unit of both trees for the device only with the flags of esvit_amd/build.py, drops what depends on the
# path or the build rather than the code (comment lines, .file / .ident / .loc, the __hip_cuid symbol) and diffs the rest: one line
# per unit with its line count and the number of differing lines, exit status 1 if any unit differs.  A plain diff of two compiler
# outputs -- the check for a change to common.h / mfma.h / gemm_kernels.h that is meant to leave every kernel as it was.
# workdir (default: a fresh temporary directory) keeps the assembly as parent/<stem>.s and new/<stem>.s; the other tree's files are
# reused if they are already there, so a second run compiles this tree only.  Stems restrict the run to those units.
set -u
[ $# -ge 1 ] && [ -d "$1/esvit_amd/csrc" ] || { echo "usage: $0 <parent-tree> [workdir [stem ...]]" >&2; exit 2; }
parent=$(cd "$1" && pwd); here=$(cd "$(dirname "$0")/.." && pwd)
work=${2:-$(mktemp -d)}; mkdir -p "$work/parent" "$work/new"; work=$(cd "$work" && pwd)
shift; [ $# -ge 1 ] && shift
stems=${*:-$(cd "$here/esvit_amd/csrc" && ls *.hip | sed 's/\.hip$//')}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}

emit() {  # tree, side, stem -> $work/side/stem.s (stripped)
    local out=$work/$2/$3.s
    [ "$2" = parent ] && [ -s "$out" ] && return 0
    (cd "$1" && "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wno-unused-result -I include -I esvit_amd/csrc \
        -x hip --cuda-device-only -S esvit_amd/csrc/$3.hip -o "$out.raw") 2> "$out.err" || { rm -f "$out"; return 1; }
    grep -v -e '^[[:space:]]*;' -e '^[[:space:]]*\.file' -e '^[[:space:]]*\.ident' -e '^[[:space:]]*\.loc' -e '__hip_cuid' "$out.raw" > "$out"
    rm -f "$out.raw" "$out.err"
}
export -f emit; export work HIPCC
for s in $stems; do printf '%s parent %s\n%s new %s\n' "$parent" "$s" "$here" "$s"; done | xargs -P "${JOBS:-8}" -L 1 bash -c 'emit "$0" "$1" "$2"'

"$HIPCC" --version | grep -i 'hip version'
bad=0
for s in $stems; do
    a=$work/parent/$s.s; b=$work/new/$s.s
    if [ ! -s "$a" ] || [ ! -s "$b" ]; then echo "$s: did not compile in $([ -s "$a" ] && echo this || echo the parent) tree ($work/*/$s.s.err)"; bad=1; continue; fi
    d=$(diff "$a" "$b" | grep -c '^[<>]')
    printf '%-28s %7d lines  %6d differing\n' "$s.hip" "$(wc -l < "$b")" "$d"
    [ "$d" -eq 0 ] || bad=1
done
[ $bad -eq 0 ] && echo "identical: every unit" || echo "DIFFERENT: see above; diff $work/parent/<stem>.s $work/new/<stem>.s"
exit $bad
