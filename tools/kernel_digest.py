#!/usr/bin/env python3
"""Per-kernel digests of the gfx950 device code, for refactors that must not change what runs (needs no GPU).

    python tools/kernel_digest.py list [BUILD_DIR] > listing.txt     one line per kernel: file, digest, lines, demangled name
    python tools/kernel_digest.py diff OLD.txt NEW.txt               the kernels whose digest differs, appeared or went away

BUILD_DIR (default go-pocket-tts_amd/build) holds the Makefile's <name>.hip.o objects.  For each, the gfx950 code object is
taken out of the .hip_fatbin section (llvm-objcopy, clang-offload-bundler --unbundle) and disassembled (llvm-objdump -d); a
kernel's digest is the sha256 of its disassembly with the address / encoding comments cut off.  A line "<file> <sha256> <bytes>
(code object)" carries the whole code object.  The disassembly is only read and hashed: nothing in it is inspected.
Two trees compare equal only if each was built by the Makefile's rule from its own go-pocket-tts_amd directory (the rule
names relative paths, so the command line, and with it the __hip_cuid_ symbol, is the same in both).
"""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def llvm_bin():
    for d in (os.environ.get("PTTS_LLVM_BIN"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),
              os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")):
        if d and os.path.exists(os.path.join(d, "llvm-objdump")):
            return d
    sys.exit("kernel_digest: llvm-objdump not found (set PTTS_LLVM_BIN)")


def code_object(llvm, obj, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None                                         # an object without device code
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fat}", f"--output={co}"], check=True)
    return co


def kernels(llvm, co):
    """[(demangled name, sha256 of the stripped disassembly, lines)] in the order of the code object"""
    text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", "-C", "--no-show-raw-insn", co], check=True,
                          capture_output=True, text=True).stdout
    out, name, body = [], None, []

    def flush():
        if name is not None:
            out.append((name, hashlib.sha256("\n".join(body).encode()).hexdigest(), len(body)))

    for line in text.splitlines():
        m = LABEL.match(line)
        if m:
            flush()
            name, body = m.group(1), []
        elif name is not None and line.strip():
            body.append(line.split("//")[0].rstrip())
    flush()
    return out


def cmd_list(build_dir):
    llvm = llvm_bin()
    objs = sorted(glob.glob(os.path.join(build_dir, "*.hip.o")))
    if not objs:
        sys.exit(f"kernel_digest: no *.hip.o under {build_dir}")
    for obj in objs:
        fname = os.path.basename(obj)[:-2]
        with tempfile.TemporaryDirectory() as tmp:
            co = code_object(llvm, obj, tmp)
            if co is None:
                continue
            with open(co, "rb") as f:
                blob = f.read()
            print(f"{fname}\t{hashlib.sha256(blob).hexdigest()}\t{len(blob)}\t(code object)")
            for name, digest, lines in kernels(llvm, co):
                print(f"{fname}\t{digest[:16]}\t{lines}\t{name}")


def read_listing(path):
    d = {}
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) == 4:
                d[(p[0], p[3])] = (p[1], p[2])
    return d


def cmd_diff(old, new):
    a, b = read_listing(old), read_listing(new)
    n = 0
    for key in sorted(set(a) | set(b)):
        if a.get(key) == b.get(key):
            continue
        n += 1
        fmt = lambda v: "absent" if v is None else f"{v[0][:16]} ({v[1]})"
        print(f"{key[0]}\t{key[1]}\t{fmt(a.get(key))} -> {fmt(b.get(key))}")
    same = sum(1 for k in a if k[1] != "(code object)" and a[k] == b.get(k))
    print(f"# {same} kernels identical, {n} entries differ", file=sys.stderr)
    return 1 if n else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("list")
    p.add_argument("build_dir", nargs="?", default=os.path.join(ROOT, "go-pocket-tts_amd", "build"))
    p = sub.add_parser("diff")
    p.add_argument("old")
    p.add_argument("new")
    args = ap.parse_args()
    if args.cmd == "list":
        cmd_list(args.build_dir)
        return 0
    return cmd_diff(args.old, args.new)


if __name__ == "__main__":
    sys.exit(main())
