#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of libmm_render.so, kernel by kernel, without a GPU.

    python tools/kernel_disasm_diff.py OLD/libmm_render.so NEW/libmm_render.so [--drop-last-false]

Every device code object embedded in each library is disassembled with llvm-objdump; per kernel symbol the instruction text (addresses,
encodings and symbol-relative branch targets removed) is hashed.  Printed: kernels whose code is identical, kernels that differ, and kernels that
exist on one side only.  With --drop-last-false a kernel of OLD that has no namesake in NEW is matched with the NEW kernel that carries one
more, trailing, `false` template argument: `pixel_bwd_kernel<true, false, false>` of OLD meets `pixel_bwd_kernel<true, false, false, false>`
of NEW.  A hand tool (exit status 1 if a kernel of OLD changed or vanished); used for profiles/render_views_headline_ab.md."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def code_objects(lib, tmp):
    """the device ELFs bundled in the host library's .hip_fatbin section"""
    fat = os.path.join(tmp, os.path.basename(lib) + ".fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    blob = open(fat, "rb").read()
    out, pos, k = [], 0, 0
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    while True:
        pos = blob.find(magic, pos)
        if pos < 0:
            break
        nxt = blob.find(magic, pos + 1)
        piece = os.path.join(tmp, "%s.bundle%d" % (os.path.basename(lib), k))
        open(piece, "wb").write(blob[pos:nxt if nxt > 0 else len(blob)])
        elf = piece + ".co"
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + piece,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf], stderr=subprocess.DEVNULL)
        if os.path.getsize(elf) > 0:
            out.append(elf)
        pos, k = pos + 1, k + 1
    return out


def kernels(lib, tmp):
    table = {}
    for elf in code_objects(lib, tmp):
        txt = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", "--no-leading-addr", elf], text=True)
        name, body = None, []
        for line in txt.splitlines() + ["<end>:"]:
            m = re.match(r"^<(.*)>:$", line.strip())
            if m:
                if name and "kernel" in name and body:
                    table[name] = (hashlib.sha1("\n".join(body).encode()).hexdigest(), len(body))
                name, body = m.group(1), []
            elif name and line.strip():
                ins = re.sub(r"//.*$", "", line).strip()
                ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<rel>", ins)      # branch targets relative to the symbol: position only
                if ins:
                    body.append(ins)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop-last-false", action="store_true", help="match NEW kernels that gained a trailing `false` template argument")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = kernels(a.old, tmp)
        new = kernels(a.new, tmp)
    if a.drop_last_false:
        for k in [k for k in old if k not in new]:
            twin = re.sub(r">\(", ", false>(", k, count=1)
            if twin != k and twin in new:
                new[k] = new.pop(twin)
    same = sorted(k for k in old if k in new and old[k] == new[k])
    diff = sorted(k for k in old if k in new and old[k] != new[k])
    print("identical machine code: %d kernels" % len(same))
    for k in same:
        print("  = %s  (%d instructions)" % (k, old[k][1]))
    print("different machine code: %d kernels" % len(diff))
    for k in diff:
        print("  ! %s  (%d -> %d instructions)" % (k, old[k][1], new[k][1]))
    print("only in OLD: %d" % len([k for k in old if k not in new]))
    for k in sorted(k for k in old if k not in new):
        print("  - %s" % k)
    print("only in NEW: %d" % len([k for k in new if k not in old]))
    for k in sorted(k for k in new if k not in old):
        print("  + %s  (%d instructions)" % (k, new[k][1]))
    return 1 if diff or any(k not in new for k in old) else 0


if __name__ == "__main__":
    sys.exit(main())
