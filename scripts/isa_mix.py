#!/usr/bin/env python3
"""Static instruction mix of one kernel instance of a translation unit of mtgp_kernels.hip.

Compiles the unit to gfx950 assembly on the CPU with the library's own flags (HIPCC_FLAGS and the
unit's flags of __graft_entry__, plus any -D / -f given here), finds the kernel whose demangled
name contains --kernel, and counts the instructions between two of its program call sites
(s_swappc_b64, in text order; default the first and the last) by class.  A counter, not a check.
The C3 instance holds several loops (RK4, Euler, the interpreter-capable one); its first five call
sites are the RK4 JIT loop's four stages and save point, so `--last 4` spans that loop's stages.

usage: isa_mix.py [--tu 7] [--kernel SUBSTR] [--first I] [--last J] [--keep FILE.s | --asm FILE.s] [-DNAME=V ...] [-fFLAG ...]
"""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

C3_KERNEL = "k_ctl_dynamic<(anonymous namespace)::EnvAcrobot, 2, true, false, true>"

CLASSES = ("valu_f32", "valu_pk_f32", "valu_other", "v_mov", "lane_rw", "s_nop", "s_waitcnt", "salu", "branch",
           "memory", "other")


def classify(op):
    if op.startswith("v_pk_") and op.endswith("_f32"):
        return "valu_pk_f32"
    if op in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32"):
        return "lane_rw"
    if op.startswith("v_mov_") or op.startswith("v_accvgpr_"):
        return "v_mov"
    if op.startswith("v_"):
        return "valu_f32" if re.search(r"_f32(_e32|_e64|_dpp|_sdwa)?$", op) else "valu_other"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_cbranch", "s_branch", "s_swappc", "s_setpc", "s_call", "s_endpgm")):
        return "branch"
    if op.startswith("s_"):
        return "salu" if not op.startswith(("s_load", "s_buffer_load")) else "memory"
    if op.startswith(("global_", "flat_", "scratch_", "ds_", "buffer_")):
        return "memory"
    return "other"


def compile_asm(tu, extra, out):
    flags = [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + list(getattr(g, "HIP_TU_FLAGS", {}).get(tu, []))
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, *extra, "--cuda-device-only", "-S", f"-DMTGP_TU={tu}",
           "-I", os.path.join(ROOT, "include"), "-I", g.CSRC, os.path.join(g.CSRC, "mtgp_kernels.hip"), "-o", out]
    subprocess.run(cmd, check=True)


def kernel_body(asm, want):
    """(mangled name, instruction lines, resource lines) of the one kernel whose demangled name contains `want`"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
    dem = subprocess.run([filt, *names], check=True, capture_output=True, text=True).stdout.splitlines()
    hits = [n for n, d in zip(names, dem) if want in d]
    if len(hits) != 1:
        raise SystemExit(f"{len(hits)} kernels match {want!r}:\n" + "\n".join(d for d in dem if want in d or not hits))
    name = hits[0]
    start = asm.index(f"\n{name}:")
    end = asm.index(".Lfunc_end", start)
    tail = asm[end:asm.index(".end_amdhsa_kernel", end)]
    res = re.findall(r"^\s*(\.amdhsa_next_free_vgpr|\.amdhsa_next_free_sgpr|\.amdhsa_private_segment_fixed_size)\s+(\S+)",
                     tail, re.M)
    res += re.findall(r"^; (Occupancy|ScratchSize|NumVgprs|NumSgprs): (\S+)", asm[end:end + 4000], re.M)
    ins = []
    for line in asm[start:end].splitlines()[2:]:
        s = line.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        ins.append(s)
    return name, ins, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tu", type=int, default=7)
    ap.add_argument("--kernel", default=C3_KERNEL)
    ap.add_argument("--first", type=int, default=0, help="index of the first call site of the span")
    ap.add_argument("--last", type=int, default=-1, help="index of the last call site of the span")
    ap.add_argument("--keep", help="write the unit's assembly here")
    ap.add_argument("--asm", help="count in this assembly file (of an earlier --keep) instead of compiling")
    a, extra = ap.parse_known_args()
    bad = [x for x in extra if not x.startswith(("-D", "-f", "-m"))]
    if bad:
        raise SystemExit(f"unknown arguments {bad}")
    with tempfile.TemporaryDirectory() as td:
        path = a.asm or a.keep or os.path.join(td, "tu.s")
        if not a.asm:
            compile_asm(a.tu, extra, path)
        with open(path) as f:
            asm = f.read()
    name, ins, res = kernel_body(asm, a.kernel)
    calls = [i for i, s in enumerate(ins) if s.startswith("s_swappc_b64")]
    print(f"kernel {a.kernel}\n  {name}\n  flags {' '.join(extra) or '(library)'}")
    print("  resources " + ", ".join(f"{k.lstrip('.')}={v}" for k, v in res))
    print(f"  {len(ins)} instructions, {len(calls)} program call sites; instructions from each site to the next: "
          + " ".join(str(b - a0) for a0, b in zip(calls, calls[1:])))
    if len(calls) < 2:
        return
    lo, hi = calls[a.first], calls[a.last]
    mix = collections.Counter(classify(s.split()[0]) for s in ins[lo:hi])
    print(f"  span: call site {a.first % len(calls)} .. {a.last % len(calls)}, {hi - lo} instructions")
    for c in CLASSES:
        print(f"    {c:12s} {mix.get(c, 0):5d}")
    scr = sum(1 for s in ins[lo:hi] if s.startswith("scratch_"))
    print(f"    (scratch accesses in the span: {scr})")


if __name__ == "__main__":
    main()
