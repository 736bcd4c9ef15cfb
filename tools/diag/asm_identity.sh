#!/bin/sh
# Device-assembly identity check of a refactor: compiles the given .hip files of two source trees to gfx950 assembly with the
# Makefile's flags and diffs them.  Usage: tools/diag/asm_identity.sh PARENT_CSRC NEW_CSRC OUT_DIR file.hip ...
# Prints per file: lines of assembly (parent, new), differing lines, differing lines that are not a .file / .loc / .ident line or the compilation-unit id (__hip_cuid_<hash of the source>),
# and whether the sets of kernel symbols (.amdhsa_kernel) are equal.
set -eu
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -fPIC -std=c++17 --offload-arch=${ARCH:-gfx950} -Wall -Wno-unused-function --cuda-device-only -S"
parent=$1; new=$2; out=$3; shift 3
mkdir -p "$out/parent" "$out/new"
for f in "$@"; do
    b=${f%.hip}
    [ -f "$out/parent/$b.s" ] || $HIPCC $FLAGS "$parent/$f" -o "$out/parent/$b.s" &
    $HIPCC $FLAGS "$new/$f" -o "$out/new/$b.s" &
done
wait
printf '%-26s %9s %9s %6s %6s %s\n' file parent new diff code kernels
for f in "$@"; do
    b=${f%.hip}
    np=$(wc -l < "$out/parent/$b.s"); nn=$(wc -l < "$out/new/$b.s")
    d=$(diff "$out/parent/$b.s" "$out/new/$b.s" | grep -c '^[<>]' || true)
    c=$(diff "$out/parent/$b.s" "$out/new/$b.s" | grep '^[<>]' | grep -vcE '^[<>][[:space:]]*\.(file|loc|ident)|__hip_cuid_' || true)
    grep '\.amdhsa_kernel' "$out/parent/$b.s" | sort > "$out/parent/$b.kernels"
    grep '\.amdhsa_kernel' "$out/new/$b.s" | sort > "$out/new/$b.kernels"
    if cmp -s "$out/parent/$b.kernels" "$out/new/$b.kernels"; then k="equal ($(wc -l < "$out/new/$b.kernels"))"; else k=DIFFERENT; fi
    printf '%-26s %9d %9d %6d %6d %s\n' "$f" "$np" "$nn" "$d" "$c" "$k"
done
