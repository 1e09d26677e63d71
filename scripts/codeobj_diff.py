"""Is the device code of two builds the same, kernel by kernel?

python scripts/codeobj_diff.py OBJDIR_A OBJDIR_B [> profiles/dispatch/codeobj_parent_vs_branch.txt]

For every object both directories hold (mtgp_kernels_tu*.o, mtgp_grad.o ...) the gfx950 code object
is unbundled (scripts/kres.py) and compared per kernel symbol: the set of kernels, each kernel's code
bytes, its kernel descriptor and its metadata entry (VGPR / SGPR / AGPR counts, spills, scratch, LDS,
kernarg size).  One line per object.  Only bytes, hashes and notes are compared; no instruction is
decoded.

A change of the host code can reorder template instantiations and so move kernels inside an object.
The whole-file hash is therefore reported but not judged, and two position-dependent items are
taken out of the comparison:
 * the descriptor's entry offset (bytes 16-23: kernel address minus descriptor address);
 * PC-relative offsets in the code of a kernel that moved.  Such a kernel counts as "moved" (and the
   same) only if its size is unchanged and every 32-bit word that differs changed by exactly
   (displacement of some symbol of the object, or 0) - (displacement of the kernel), i.e. it is the
   distance to a table or function that kept its contents.  Anything else is "DIFFERENT"."""
import glob
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402

META = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def sections(data):
    """(address, file offset, size) of every section of an ELF64 little-endian image."""
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    out = []
    for i in range(shnum):
        addr, off, size = struct.unpack_from("<QQQ", data, shoff + i * shentsize + 0x10)
        out.append((addr, off, size))
    return out


def code_object_symbols(obj):
    """{symbol: (address, bytes)} of the defined functions and objects, {kernel: metadata tuple},
    whole code-object sha."""
    with tempfile.TemporaryDirectory() as tmp:
        co = kres.code_object(obj, tmp)
        data = open(co, "rb").read()
        meta = {k["name"]: tuple(k.get(f, 0) for f in META) for k in kres.kernels_of(co)}
        syms = subprocess.run([f"{kres.LLVM}/llvm-readelf", "--dyn-syms", "-W", co], check=True, capture_output=True,
                              text=True).stdout
    secs = sections(data)
    sym = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, size, sec = int(f[1], 16), int(f[2]), secs[int(f[6])]
            sym[f[7]] = (addr, data[sec[1] + addr - sec[0]:sec[1] + addr - sec[0] + size])
    return sym, meta, hashlib.sha256(data).hexdigest()


def same_code(ka, kb, shifts):
    """'same' (byte for byte), 'moved' (see the module text) or 'differs'."""
    (addr_a, code_a), (addr_b, code_b) = ka, kb
    if code_a == code_b:
        return "same"
    if len(code_a) != len(code_b) or len(code_a) % 4 or addr_a == addr_b:
        return "differs"
    n = len(code_a) // 4
    allowed = {(t - (addr_b - addr_a)) & 0xFFFFFFFF for t in shifts | {0}}
    for x, y in zip(struct.unpack(f"<{n}I", code_a), struct.unpack(f"<{n}I", code_b)):
        if x != y and ((y - x) & 0xFFFFFFFF) not in allowed:
            return "differs"
    return "moved"


def descriptor_sha(kd):
    return hashlib.sha256(kd[:16] + bytes(8) + kd[24:]).hexdigest()


def main(dir_a, dir_b):
    names = sorted({os.path.basename(p) for p in glob.glob(os.path.join(dir_a, "*.o"))} &
                   {os.path.basename(p) for p in glob.glob(os.path.join(dir_b, "*.o"))})
    bad = compared = 0
    for name in names:
        try:
            sa, ma, file_a = code_object_symbols(os.path.join(dir_a, name))
            sb, mb, file_b = code_object_symbols(os.path.join(dir_b, name))
        except subprocess.CalledProcessError:
            continue  # a host-only object: no device code to compare
        compared += 1
        ka, kb = ({s[:-3] for s in sym if s.endswith(".kd")} for sym in (sa, sb))
        only, both = sorted(ka ^ kb), sorted(ka & kb)
        shifts = {sb[s][0] - sa[s][0] for s in set(sa) & set(sb)}
        code = {k: same_code(sa[k], sb[k], shifts) for k in both}
        kd = [k for k in both if descriptor_sha(sa[k + ".kd"][1]) != descriptor_sha(sb[k + ".kd"][1])]
        md = [k for k in both if ma[k] != mb[k]]
        count = {v: sum(1 for c in code.values() if c == v) for v in ("same", "moved", "differs")}
        ok = not only and not kd and not md and not count["differs"]
        bad += not ok
        print(f"{name}: {len(ka)} vs {len(kb)} kernels, symbol sets {'equal' if not only else 'DIFFER'}; code "
              f"byte-identical {count['same']}, moved {count['moved']}, differs {count['differs']}; descriptor differs "
              f"{len(kd)}; metadata differs {len(md)}; whole file {'equal' if file_a == file_b else 'differs'} -- "
              f"{'SAME' if ok else 'DIFFERENT'}")
        for k in only + sorted({k for k in both if code[k] == "differs"} | set(kd) | set(md)):
            print(f"    {k}")
    return 1 if bad or not compared else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
