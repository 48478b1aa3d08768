#!/usr/bin/env python3
"""Compare the kernels of gfx950 code objects function by function.

Usage: tools/kcmp.py [--rename 'OLD_PREFIX=NEW_PREFIX' ...] OLD.co NEW.co [NEW2.co ...]

Each argument is a device code object (hipcc --offload-device-only -c, as tools/kres.sh builds
one) or an offload bundle, which is unbundled for gfx950 first.  The kernels of the NEW objects
together are compared with OLD's: every kernel (a function with a `.kd` descriptor) is
disassembled with llvm-objdump -d and its whole text -- mnemonics, operands and encodings, the
address column dropped -- must match.  A kernel's own symbol in the comments of its branches
(`<symbol+0x...>`) is dropped too, so a renamed kernel still compares, and so is the `s_nop 0`
padding behind a kernel's last instruction (it fills the gap to the next symbol or to the section's
end, so it depends on which kernel follows in the object, not on the kernel).  --rename (repeatable)
replaces OLD_PREFIX at the start of OLD's demangled kernel names by NEW_PREFIX before the names are
matched, for kernels that were renamed or whose template list changed.  Prints the identical, differing, missing (only in OLD) and
added (only in NEW) kernels, a kernel found in two NEW objects, and exits 1 unless every kernel of
NEW is identical to OLD's.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hip-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(path, tmp):
    with open(path, "rb") as f:
        bundle = f.read(24) == b"__CLANG_OFFLOAD_BUNDLE__"
    if not bundle:
        return path
    out = os.path.join(tmp, os.path.basename(path) + ".gfx950")
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}",
        f"--input={path}", f"--output={out}")
    return out


def kernels(path, tmp):
    """{demangled kernel name: its disassembly without addresses} of one code object."""
    co = code_object(path, tmp)
    syms = run(f"{LLVM}/llvm-readelf", "-sW", co)
    kds = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.rstrip().endswith(".kd")}
    funcs, name = {}, None
    for ln in run(f"{LLVM}/llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif name is not None and ln.strip() and ln.strip() != "...":  # "...": zero padding up to the next symbol
            # "\tinsn operands  // 000000001234: ENCODING ..." -> drop the address
            ln = re.sub(r"//\s*[0-9A-Fa-f]+:", "//", ln).strip()
            funcs[name].append(ln.replace(f"<{name}+", "<+"))  # branch targets: offset only
    for text in funcs.values():  # s_nop padding behind the last instruction, up to the next symbol or the
        while text and text[-1].split("//")[0].strip() == "s_nop 0":  # section's end: not part of the function
            text.pop()
    names = sorted(kds)
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    pretty = run(filt, *names).splitlines() if names and filt else names
    return {p: "\n".join(funcs.get(n, ["<no text>"])) for n, p in zip(names, pretty)}


def renamed(name, renames):
    for a, b in renames:
        if name.startswith(a):
            return b + name[len(a):]
    return name


def main(argv):
    renames = []
    while len(argv) > 2 and argv[1] == "--rename":
        a, sep, b = argv[2].partition("=")
        if not sep:
            sys.exit(__doc__)
        renames.append((a, b))
        del argv[1:3]
    if len(argv) < 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old = {renamed(k, renames): text for k, text in kernels(argv[1], tmp).items()}
        new, twice = {}, []
        for p in argv[2:]:
            for k, text in kernels(p, tmp).items():
                if k in new:
                    twice.append(k)
                new[k] = text
    same = [k for k in new if k in old and new[k] == old[k]]
    differ = [k for k in new if k in old and new[k] != old[k]]
    missing = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    for title, ks in (("identical", same), ("differing", differ), ("missing", missing), ("added", added),
                      ("in two objects", twice)):
        print(f"{title}: {len(ks)}")
        for k in sorted(ks):
            print(f"  {k}")
    return 0 if not (differ or added or twice) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
