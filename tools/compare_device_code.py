#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same, symbol by symbol?

    python tools/compare_device_code.py OLD_DIR NEW_DIR [--arch gfx950]

OLD_DIR / NEW_DIR hold the object files of two builds of textflux_amd/csrc (`make` and `make bench` objects: *.o).  For every
object name present in either directory the .hip_fatbin section is extracted, the hipv4-amdgcn-amd-amdhsa--<arch> code object
unbundled, and compared per symbol: the set of FUNC symbols and *.kd kernel descriptors, the bytes of each, and the notes
(register counts, LDS, scratch, kernarg layout).  The __hip_cuid_<hash> symbol is derived from the source text and is ignored.
Comparing per symbol keeps the check valid when a host-side edit changes the order in which templates are first instantiated:
the two things that follow that order -- the entry offset inside a kernel descriptor and the sequence of the per-kernel metadata
records -- are compared as "points at its own kernel" and as a sorted list.
Needs no GPU.  Exit status 0 = nothing differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, arch, tmp):
    """path of the unbundled device ELF of `obj`, or None when it carries no device code"""
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    co = fat + ".co"
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
        f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}")
    return co if os.path.getsize(co) else None


def symbols(co):
    """{name: (kind, bytes)} of the FUNC symbols and the kernel descriptors of a code object"""
    sections = {}   # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-S", "-W", co), re.M):
        sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    blob = open(co, "rb").read()
    out = {}
    for line in run(f"{LLVM}/llvm-readelf", "-s", "-W", co).splitlines():
        f = line.split()
        if len(f) < 8 or not f[0].rstrip(":").isdigit() or not f[6].isdigit():
            continue
        value, size, kind, name, shndx = int(f[1], 16), int(f[2]), f[3], f[7], int(f[6])
        if name.startswith("__hip_cuid_") or not (kind == "FUNC" or name.endswith(".kd")):
            continue
        addr, off = sections[shndx]
        start = off + value - addr
        out[name] = (kind, value, blob[start:start + size])
    # A kernel descriptor holds the distance to its kernel's entry (kernel_code_entry_byte_offset, bytes 16 .. 23), which moves with the
    # order of the functions in .text: check that it points at the kernel's own code, then compare the descriptor without it.
    address = {name: value for name, (_, value, _) in out.items()}
    for name, (kind, value, data) in out.items():
        if name.endswith(".kd") and len(data) == 64:
            entry = value + int.from_bytes(data[16:24], "little", signed=True)
            target = "own kernel" if address.get(name[:-3]) == entry else f"entry {entry:#x}"
            data = data[:16] + target.encode() + data[24:]
        out[name] = (kind, data)
    return out


def notes(co):
    """the notes with the per-kernel metadata records sorted (their order is the order of the functions in .text)"""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", run(f"{LLVM}/llvm-readelf", "--notes", co))
    head, kernels, tail, where = [], [], [], "head"
    for line in text.splitlines():
        if where == "head":
            head.append(line)
            if line.strip() == "amdhsa.kernels:":
                where = "kernels"
        elif where == "kernels" and line.startswith("  - "):
            kernels.append([line])
        elif where == "kernels" and line.startswith("    ") and kernels:
            kernels[-1].append(line)
        else:
            where = "tail"
            tail.append(line)
    return head, sorted(kernels), tail


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    names = sorted({f for d in (a.old, a.new) for f in os.listdir(d) if f.endswith(".o")})
    bad = 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        for n in names:
            paths = [os.path.join(d, n) for d in (a.old, a.new)]
            if not all(os.path.exists(p) for p in paths):
                # an object one build does not have (host code moved between files) is no difference as long as it holds no kernels
                path, tmp = [(p, t) for p, t in zip(paths, (t_old, t_new)) if os.path.exists(p)][0]
                host_only = code_object(path, a.arch, tmp) is None
                print(f"{n}: present in one build only, {'no device code' if host_only else 'WITH device code'}")
                bad += not host_only
                continue
            co = [code_object(p, a.arch, t) for p, t in zip(paths, (t_old, t_new))]
            if co[0] is None and co[1] is None:
                print(f"{n}: no device code")
                continue
            if co[0] is None or co[1] is None:
                print(f"{n}: device code in one build only")
                bad += 1
                continue
            so, sn = symbols(co[0]), symbols(co[1])
            differing = sorted(set(so) ^ set(sn)) + sorted(k for k in set(so) & set(sn) if so[k] != sn[k])
            notes_equal = notes(co[0]) == notes(co[1])
            kernels = sum(1 for k in sn if k.endswith(".kd"))
            print(f"{n}: {kernels} kernels, {len(sn)} symbols compared, differing: {', '.join(differing) if differing else 'none'}, "
                  f"notes {'equal' if notes_equal else 'DIFFER'}")
            bad += len(differing) + (not notes_equal)
    print("device code identical" if not bad else f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
