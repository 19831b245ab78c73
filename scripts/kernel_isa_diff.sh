#!/bin/bash
# Instruction-for-instruction comparison of the gfx950 kernels of two built objects (no GPU needed):
#   bash scripts/kernel_isa_diff.sh [--demangled] A.o B.o
# --demangled pairs the kernels by demangled name with "(anonymous namespace)::" removed instead of by symbol: for a
# change that moves kernels between an anonymous namespace and its parent, which renames every symbol.
# Per kernel symbol present in both, the disassemblies (llvm-objdump -d) are compared after masking what moves when
# other code of the object comes or goes:
#   - the trailing "// address: encoding" comments;
#   - the numeric ids inside local labels (LBB<n>_, and the %= ids of inline-asm labels such as LP<n>_0, LG<n>);
#   - the literal of the s_add_u32 that follows an s_getpc_b64 (a PC-relative distance to read-only data);
#   - the alignment padding after a kernel's last instruction (s_nop 0, s_code_end, and the "..." llvm-objdump prints
#     for a run of zero bytes).
# Prints the kernels only in A, only in B, and those that differ; exit status 1 when a common kernel differs.
set -o pipefail
PAIR=symbol
if [ "$1" = --demangled ]; then PAIR=demangled; shift; fi
[ $# -eq 2 ] || { echo "usage: $0 [--demangled] A.o B.o" >&2; exit 2; }
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
L=/opt/rocm/lib/llvm/bin
for s in a b; do
    if [ $s = a ]; then OBJ=$(realpath "$1"); else OBJ=$(realpath "$2"); fi
    $L/llvm-objcopy --dump-section .hip_fatbin="$T/$s.fat" "$OBJ" && \
    $L/clang-offload-bundler --unbundle --type=o --input="$T/$s.fat" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$T/$s.co" && \
    $L/llvm-readelf -sW "$T/$s.co" | awk '$4 == "FUNC" && $7 != "UND" {print $8}' > "$T/$s.funcs" && \
    $L/llvm-objdump -d "$T/$s.co" > "$T/$s.dis" || exit 2
done
python3 - "$T" $PAIR <<'EOF'
import re, subprocess, sys
T, PAIR = sys.argv[1:3]
HEAD = re.compile(r"^[0-9a-f]+ <(.+)>:$")
LABEL = re.compile(r"\b(L[A-Z]+)\d+")
LIT = re.compile(r"(s_add_u32\s+\S+,\s*\S+,\s*)\S+")


def kernels(s):
    funcs = set(open(f"{T}/{s}.funcs").read().split())
    out, cur, getpc = {}, None, False
    for line in open(f"{T}/{s}.dis"):
        m = HEAD.match(line.strip())
        if m and m.group(1) in funcs:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        line = LABEL.sub(r"\1#", (m.group(1) + ":") if m else line.split("//")[0].strip())  # (a local label: no address)
        if not line:
            continue
        if getpc and line.startswith("s_add_u32"):
            line = LIT.sub(r"\1<pcrel>", line)
        getpc = line.startswith("s_getpc_b64")
        cur.append(line)
    for body in out.values():  # (the padding after a kernel's last instruction depends on where the next one starts)
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):  # ("...": llvm-objdump's run of zero bytes)
            body.pop()
    if PAIR == "demangled":
        names = list(out)
        plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        out = {d.replace("(anonymous namespace)::", ""): out[n] for n, d in zip(names, plain)}
        assert len(out) == len(names), "two kernels share a demangled name"
    return out


a, b = kernels("a"), kernels("b")
for name in sorted(set(a) - set(b)):
    print("only in A:", name)
for name in sorted(set(b) - set(a)):
    print("only in B:", name)
differ = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
for name in differ:
    at = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
    print(f"differs: {name}  ({len(a[name])} / {len(b[name])} instructions, first at {at})")
    print("    A:", " | ".join(a[name][at:at + 3]))
    print("    B:", " | ".join(b[name][at:at + 3]))
print(f"{len(a)} kernels in A, {len(b)} in B, {len(set(a) & set(b))} in both, {len(differ)} differ")
sys.exit(1 if differ else 0)
EOF
