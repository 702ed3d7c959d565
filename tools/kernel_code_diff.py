#!/usr/bin/env python3
"""Diagnostic: do two builds of a translation unit hold the same gfx950 code for the kernels they share?
   python tools/kernel_code_diff.py PARENT.o THIS.o        (objects or libraries with one offload bundle, e.g. lib/obj/bb_engine.o)
Disassembles both code objects (llvm-objdump -d) and compares kernel by kernel, by name.  Adding a kernel moves the others inside
the code object, so three things are masked that say nothing about a kernel's own instructions: addresses and encodings, the
literal of the `s_add_u32` that follows `s_getpc_b64` (the pc-relative distance to a constant table), and padding after the last
instruction.  Prints the kernels only one side has and those whose instructions differ; exit status 1 if any shared kernel differs."""
import difflib
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


def code_object(path):
    data = open(path, "rb").read()
    o = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    if o < 0:
        raise SystemExit(f"{path}: no offload bundle")
    n = struct.unpack_from("<Q", data, o + 24)[0]
    p = o + 32
    for _ in range(n):
        off, size, tl = struct.unpack_from("<QQQ", data, p)
        p += 24
        trip = data[p:p + tl].decode()
        p += tl
        if "gfx950" in trip and size:
            return data[o + off:o + off + size]
    raise SystemExit(f"{path}: no gfx950 code object")


def kernels(path):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object(path))
        f.flush()
        txt = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            cur.append(line.split("//")[0].rstrip())
    for name, ls in out.items():
        for i in range(1, len(ls)):
            if "s_getpc_b64" in ls[i - 1] and "s_add_u32" in ls[i]:
                ls[i] = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ls[i])
        while ls and (not ls[-1].strip() or ls[-1].strip() == "..." or "s_nop" in ls[-1] or "s_code_end" in ls[-1]):
            ls.pop()
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}")
    for k in sorted(set(a) - set(b)):
        print("only in the first :", k)
    for k in sorted(set(b) - set(a)):
        print("only in the second:", k)
    bad = [k for k in a if k in b and a[k] != b[k]]
    for k in bad:
        d = [l for l in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        print(f"DIFFERS: {k} ({len(d)} lines)")
        print("\n".join(d[:12]))
    print(f"{len(set(a) & set(b)) - len(bad)} shared kernels identical, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
