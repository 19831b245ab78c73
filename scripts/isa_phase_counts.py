#!/usr/bin/env python3
"""Static instruction counts of the shading phase of a render_drain instantiation (DESIGN.md §38's counting rule).

The rule: the instructions after the walk's `s_setprio 0` up to and including the drain's `s_barrier` (near half), or
up to the last `s_endpgm` (far half), in `llvm-objdump -d` of the megakernel's gfx950 code object; VALU = mnemonics
`v_*`, scalar = `s_*`, branches = `s_cbranch_*`, f64 = mnemonics with `_f64`.

    python scripts/isa_phase_counts.py raytracer-go_amd/build/rtx_kernel.o [more objects ...]
"""
import argparse
import os
import re
import subprocess
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
HEADLINE = "void rtxd::render_drain<true, 12, 6, false, true, false, false, false>(rtxd::DrainArgs)"


def disassemble(obj):
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "k.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
        return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", "--no-show-raw-insn", co], check=True,
                              capture_output=True, text=True).stdout


def kernel(text, name):
    out, on = [], False
    for line in text.splitlines():
        if line.rstrip().endswith(f"<{name}>:"):
            on = True
        elif on:
            if re.match(r"^[0-9a-f]+ <(void |\w+::|_Z)", line):  # the next kernel (local labels are <L...>)
                break
            m = re.match(r"^\s+(\S+)\s*(.*?)\s*(//.*)?$", line)
            if m and not line.rstrip().endswith(":"):
                out.append((m.group(1), m.group(2)))
    return out


def count(ins):
    def c(f):
        return sum(1 for m, _ in ins if f(m))
    return {"instr": len(ins), "VALU": c(lambda m: m.startswith("v_")), "scalar": c(lambda m: m.startswith("s_")),
            "s_load": c(lambda m: m.startswith("s_load")), "s_waitcnt": c(lambda m: m == "s_waitcnt"),
            "v_readlane": c(lambda m: m.startswith("v_readlane")), "s_nop": c(lambda m: m == "s_nop"),
            "v_mov": c(lambda m: m.startswith("v_mov")), "branches": c(lambda m: m.startswith("s_cbranch")),
            "s_branch": c(lambda m: m == "s_branch"), "f64": c(lambda m: "_f64" in m),
            "v_div": c(lambda m: m.startswith("v_div_")), "v_mad_u64_u32": c(lambda m: m == "v_mad_u64_u32"),
            "v_bitop3": c(lambda m: m.startswith("v_bitop3")), "s_add_i32": c(lambda m: m == "s_add_i32"),
            "ds_permute": c(lambda m: m.startswith(("ds_permute", "ds_bpermute"))),
            "scratch": c(lambda m: m.startswith("scratch_"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("objects", nargs="+")
    ap.add_argument("--kernel", default=HEADLINE)
    args = ap.parse_args()
    for obj in args.objects:
        k = kernel(disassemble(obj), args.kernel)
        prio0 = [i for i, (m, o) in enumerate(k) if m == "s_setprio" and o.strip() == "0"]
        bars = [i for i, (m, _) in enumerate(k) if m == "s_barrier"]
        ends = [i for i, (m, _) in enumerate(k) if m == "s_endpgm"]
        assert len(prio0) == 2 and ends, (len(k), prio0, ends)
        near = k[prio0[0] + 1:next(b for b in bars if b > prio0[0]) + 1]
        far = k[prio0[1] + 1:ends[-1] + 1]
        print(obj, "kernel instructions:", len(k))
        print("  near", count(near))
        print("  far ", count(far))


if __name__ == "__main__":
    main()
