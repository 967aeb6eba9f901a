#!/usr/bin/env python3
"""Disassemble the gfx950 code object embedded in a hipcc object file and count
instructions per kernel / per region.  Diagnostic only.

usage: tools/isa_dump.py <file.o> <out.dis> [kernel_substring]
       tools/isa_dump.py --compare <a.o> <b.o>
Extracts .hip_fatbin (an uncompressed clang offload bundle), writes the gfx950
code object next to <out.dis>, disassembles it with llvm-objdump and, when a
kernel substring is given, prints that kernel's instruction histogram.

--compare: the check that a host-side change left device code alone.  Prints
the symbols only one of the two objects has and the symbols whose instruction
text (mnemonics and operands; addresses and encodings stripped) differs, and
exits 1 if there are any."""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def extract(obj, co_path):
    fat = co_path + ".fatbin"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    assert data.startswith(magic), "compressed or unknown bundle format"
    (nb,) = struct.unpack_from("<Q", data, len(magic))
    pos = len(magic) + 8
    for _ in range(nb):
        off, size, tl = struct.unpack_from("<QQQ", data, pos)
        pos += 24
        triple = data[pos:pos + tl].decode()
        pos += tl
        if "gfx950" in triple:
            open(co_path, "wb").write(data[off:off + size])
            return
    raise SystemExit("no gfx950 bundle")


def disassemble(obj, out):
    co = out + ".co"
    extract(obj, co)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True,
                         check=True).stdout
    open(out, "w").write(dis)
    return dis


def symbols(obj, tmp, tag):
    """{symbol: its instruction lines, without the address / encoding comment}"""
    syms, cur = {}, None
    for line in disassemble(obj, os.path.join(tmp, tag + ".dis")).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(" ".join(line.split("//")[0].split()))
    return syms


def compare(obj_a, obj_b):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = symbols(obj_a, tmp, "a"), symbols(obj_b, tmp, "b")
    only = [(obj_a, s) for s in a if s not in b] + [(obj_b, s) for s in b if s not in a]
    differ = [s for s in a if s in b and a[s] != b[s]]
    for obj, s in only:
        print(f"only in {obj}: {s}")
    for s in differ:
        print(f"differs: {s} ({len(a[s])} / {len(b[s])} instructions)")
    print(f"{len(a)} / {len(b)} symbols, {len(only)} in one file only, {len(differ)} differing")
    return 1 if only or differ else 0


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    obj, out = sys.argv[1], sys.argv[2]
    dis = disassemble(obj, out)
    if len(sys.argv) > 3:
        pat = sys.argv[3]
        cur, hist = None, collections.Counter()
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
            if m:
                cur = m.group(1)
                continue
            if cur and pat in cur:
                t = line.strip().split()
                if t and re.match(r"^[a-z_0-9]+$", t[0]):
                    hist[t[0]] += 1
        v = sum(c for k, c in hist.items() if k.startswith("v_"))
        print(f"VALU {v}  SALU {sum(c for k, c in hist.items() if k.startswith('s_'))}  "
              f"LDS {sum(c for k, c in hist.items() if k.startswith('ds_'))}")
        for k, c in hist.most_common(40):
            print(f"{c:7d} {k}")


if __name__ == "__main__":
    main()
