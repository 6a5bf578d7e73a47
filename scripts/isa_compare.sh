#!/bin/bash
# Device assembly of two source trees, kernel by kernel: the proof that a refactor
# left the shipped device code alone. Runs without a GPU.
#
#   bash scripts/isa_compare.sh [-o OUT] [-j N] [-f "a.hip b.hip"] [-m "a.hip=a.hip+b.hip"] TREE_A TREE_B [extra hipcc flags]
#
# Compiles every source in SRCS of each tree's m2_mixer_amd/csrc/Makefile (or those given
# with -f) with that Makefile's CXXFLAGS, the extra flags and `--offload-device-only -S`,
# into OUT/a and OUT/b (default: a fresh temporary directory; an assembly file newer than
# its source and every header is reused).  Prints, per file, the kernel count of each tree and
# "identical" or "differs: <kernel>" with what the kernel uses in each tree (instructions, registers, spills, LDS, scratch).
# -m: TREE_B has split a.hip into the files named; they are compiled in its place and compared as their union, where data objects
# and "<other>" lines (which follow a file's sections) are printed without failing the run.
#
# Compared per function: the symbol name; the instruction text with `;` comments stripped
# and the function index of local labels (.LBB<n>_<m>, .Lfunc_end<n>) dropped; for kernels
# also the .amdhsa_ descriptor block and the kernel's entry in the amdgpu_metadata note
# (registers, LDS, scratch, kernel-argument layout).  Data objects are compared by name (their
# order in a section is an accident of the compiler's hash tables: it changes with the length
# of a comment), the remaining lines (.set lines, the rest of the note) as "<other>".  `__hip_cuid_<hash>` is a
# hash of the source and is ignored.  Text is compared; nothing is searched for.
# Exit status: 0 all identical, 1 something differs, 2 usage or a failed compile.
set -u -o pipefail
usage() { sed -n '5p' "$0" | cut -c3-; exit 2; }
out=""; jobs=4; only=""; map=""
while getopts "o:j:f:m:" opt; do
  case $opt in
    o) out=$OPTARG ;;
    j) jobs=$OPTARG ;;
    f) only=$OPTARG ;;
    m) map=$OPTARG ;;
    *) usage ;;
  esac
done
shift $((OPTIND - 1))
[ $# -ge 2 ] || usage
tree_a=$(cd "$1" && pwd) || exit 2
tree_b=$(cd "$2" && pwd) || exit 2
shift 2
extra="$*"
[ -n "$out" ] || out=$(mktemp -d)
mkdir -p "$out/a" "$out/b"
out=$(cd "$out" && pwd)
export HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}

mkvar() { sed -n "s/^$2 := //p" "$1/m2_mixer_amd/csrc/Makefile" | head -1; }
srcs=${only:-$(mkvar "$tree_a" SRCS)}
pairs=$(for s in $srcs; do [ "$s" = "${map%%=*}" ] && echo "$map" || echo "$s"; done)       # a.hip, or a.hip=its successors in TREE_B
srcs_b=$(for s in $pairs; do echo "${s#*=}" | tr '+' ' '; done)

todo() {  # one "size, directory, source, assembly file, flags" line per assembly file that is missing or stale
  local side=$1 csrc=$2/m2_mixer_amd/csrc flags s asm
  flags="$(mkvar "$2" CXXFLAGS | sed 's/\$(ARCH)/gfx950/') $extra"
  for s in $3; do
    asm=$out/$side/${s%.hip}.s
    [ -s "$asm" ] && [ -z "$(find "$csrc" -maxdepth 1 \( -name "$s" -o -name '*.h' \) -newer "$asm")" ] && continue
    rm -f "$asm"
    printf '%s\t%s\t%s\t%s\t%s\n' "$(wc -c < "$csrc/$s")" "$csrc" "$s" "$asm" "$flags"
  done
}
# (largest translation units first, so that the pool drains evenly)
{ todo a "$tree_a" "$srcs"; todo b "$tree_b" "$srcs_b"; } | sort -rn | cut -f2- | xargs -r -d '\n' -P "$jobs" -n 1 bash -c '
  IFS="	" read -r csrc s asm flags <<< "$0"
  cd "$csrc" && $HIPCC $flags --offload-device-only -S -o "$asm.tmp" "$s" 2> "$asm.log" && mv "$asm.tmp" "$asm" ||
    { echo "compile failed: $csrc/$s (see $asm.log)" >&2; exit 255; }
' || exit 2

exec python3 "$(dirname "$0")/isa_compare.py" "$out" $pairs
