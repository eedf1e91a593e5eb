#!/usr/bin/env python3
"""One line per gfx950 kernel of a built libmhla_hip.so: a hash of the kernel's machine code, its resources, its symbol.

    python tools/kernel_fingerprints.py [mhla_amd/lib/libmhla_hip.so] > fingerprints.txt
    python tools/kernel_fingerprints.py --compare parent.txt this.txt
    python tools/kernel_fingerprints.py --label-log fingerprints.txt < launches.log > labelled.log

Line: `<sha256[:16] of the kernel's bytes in .text> v<VGPRs> s<SGPRs> lds<bytes> scratch<bytes> kernarg<bytes> <mangled symbol>`.  A refactor
that renames template parameters changes the symbols and must not change anything else: --compare ignores the names and compares the
multisets of (hash, resources) and the number of kernels.  The code objects come out of the library with `llvm-objdump --offloading`
(one per translation unit); symbols and .text are read from the ELF directly, the resources from its NT_AMDGPU_METADATA note.
--label-log replaces the host-side kernel symbol of every LAUNCH line of a tools/record_launches.py log by the code hash of that tree's
kernel, so that the logs of two trees whose kernels were renamed compare with `diff`.
"""
import collections
import glob
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import msgpack

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(HERE), "mhla_amd", "lib", "libmhla_hip.so")


def objdump_path():
    for cand in (os.environ.get("LLVM_OBJDUMP"), "/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("llvm-objdump not found (looked at $LLVM_OBJDUMP, /opt/rocm/llvm/bin, PATH)")


def code_objects(lib):
    """The gfx950 code objects of `lib`, as bytes, in the order of its translation units."""
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")   # (the bundles are written beside the file they come from)
        shutil.copy(lib, copy)
        subprocess.run([objdump_path(), "--offloading", copy], check=True, stdout=subprocess.DEVNULL)
        files = sorted(glob.glob(copy + ".*gfx950*"), key=lambda f: int(f[len(copy) + 1:].split(".")[0]))
        return [open(f, "rb").read() for f in files]


def sections(elf):
    assert elf[:5] == b"\x7fELF\x02", "not a 64-bit ELF"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    raw = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    strtab = raw[shstrndx]
    name = lambda off: elf[strtab[4] + off:elf.index(b"\0", strtab[4] + off)].decode()
    return [dict(name=name(s[0]), type=s[1], addr=s[3], offset=s[4], size=s[5], link=s[6], entsize=s[9]) for s in raw]


def kernel_metadata(elf, secs):
    """symbol -> the kernel's entry of amdhsa.kernels"""
    for s in secs:
        if s["type"] != 7:   # SHT_NOTE
            continue
        pos, end = s["offset"], s["offset"] + s["size"]
        while pos < end:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, pos)
            desc = pos + 12 + (namesz + 3) // 4 * 4
            if ntype == 32 and elf[pos + 12:pos + 12 + namesz].rstrip(b"\0") == b"AMDGPU":
                meta = msgpack.unpackb(elf[desc:desc + descsz], raw=False, strict_map_key=False)
                return {k[".name"]: k for k in meta["amdhsa.kernels"]}
            pos = desc + (descsz + 3) // 4 * 4
    return {}


def fingerprints(elf):
    secs = sections(elf)
    meta = kernel_metadata(elf, secs)
    symtab = next(s for s in secs if s["type"] == 2)   # SHT_SYMTAB
    strs = secs[symtab["link"]]
    out = []
    for i in range(symtab["size"] // symtab["entsize"]):
        st_name, st_info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, symtab["offset"] + i * symtab["entsize"])
        if st_info & 15 != 2 or shndx == 0 or shndx >= len(secs):   # STT_FUNC, defined
            continue
        name = elf[strs["offset"] + st_name:elf.index(b"\0", strs["offset"] + st_name)].decode()
        if name not in meta:   # (device functions that were not inlined)
            continue
        sec, k = secs[shndx], meta[name]
        start = sec["offset"] + value - sec["addr"]
        out.append("%s v%d s%d lds%d scratch%d kernarg%d %s" % (
            hashlib.sha256(elf[start:start + size]).hexdigest()[:16], k[".vgpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"],
            k[".private_segment_fixed_size"], k[".kernarg_segment_size"], name))
    assert len(out) == len(meta), "a kernel of the metadata has no code symbol"
    return out


def without_names(path):
    return collections.Counter(line.rsplit(" ", 1)[0] for line in open(path).read().splitlines() if line.strip())


def compare(a, b):
    ca, cb = without_names(a), without_names(b)
    print("%s: %d kernels, %d distinct code hashes" % (a, sum(ca.values()), len({k.split()[0] for k in ca})))
    print("%s: %d kernels, %d distinct code hashes" % (b, sum(cb.values()), len({k.split()[0] for k in cb})))
    for k, n in sorted((ca - cb).items()):
        print("only in %s (x%d): %s" % (a, n, k))
    for k, n in sorted((cb - ca).items()):
        print("only in %s (x%d): %s" % (b, n, k))
    same = ca == cb
    print("identical multisets of (code hash, resources)" if same else "DIFFERENT")
    return 0 if same else 1


def label_log(fp_path):
    """LAUNCH name <host symbol> ... -> LAUNCH name <code hash> ...; the host symbol is the kernel's with `__device_stub__` in front of its name"""
    codes = collections.defaultdict(set)   # (a kernel that two units instantiate may be compiled differently in each: all its hashes)
    for line in open(fp_path).read().splitlines():
        codes[line.rsplit(" ", 1)[1]].add(line.split()[0])
    code = {sym: "|".join(sorted(hs)) for sym, hs in codes.items()}
    stub = re.compile(r"(\d+)__device_stub__")
    for line in sys.stdin:
        f = line.split(" ")
        if f[0] == "LAUNCH":
            f[2] = code[stub.sub(lambda m: str(int(m.group(1)) - 15), f[2], count=1)]
        sys.stdout.write(" ".join(f))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--label-log":
        sys.exit(label_log(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    for obj in code_objects(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB):
        print("\n".join(fingerprints(obj)))
