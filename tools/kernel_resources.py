#!/usr/bin/env python3
"""Registers, spills and LDS of every kernel in the gfx950 code objects bundled in a shared library (the .note metadata), and a
hash of every kernel's disassembled instructions, so that two builds can be compared kernel by kernel.

    python tools/kernel_resources.py [grid_fed_rl_gym_amd/libgridstep.so] [name filter]
    python tools/kernel_resources.py --hash [lib.so] [name filter]      also the instruction count and the hash
    python tools/kernel_resources.py --diff old.so new.so               the kernels whose hash or resources differ; exit status 1 if any

The hash covers the instructions and their operands alone (no addresses, no encodings), symbol by symbol: a refactor that leaves a
kernel's code as it was leaves its hash as it was, whatever moved around it.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "grid_fed_rl_gym_amd", "libgridstep.so")
FIELDS = ("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds")


def _code_objects(lib, tmp):
    """The library's gfx950 code objects, extracted into `tmp`."""
    work = os.path.join(tmp, os.path.basename(lib))
    shutil.copy(lib, work)
    subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", work], cwd=tmp, check=True, capture_output=True)
    return [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "gfx950" in f]


def _notes(obj, out):
    txt = subprocess.run([os.path.join(LLVM_BIN, "llvm-readobj"), "--notes", obj], capture_output=True, text=True).stdout
    for blk in txt.split("- .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
        num = lambda v: int(v) if v.isdigit() else -1
        out[g("name")] = dict(vgpr=num(g("vgpr_count")), agpr=num(blk.split()[0]), sgpr=num(g("sgpr_count")), vspill=num(g("vgpr_spill_count")),
                              sspill=num(g("sgpr_spill_count")), scratch=num(g("private_segment_fixed_size")), lds=num(g("group_segment_fixed_size")))


def _disassembly(obj, out):
    """out[symbol] = (instructions, sha256 of their text) for every symbol of the object's code."""
    txt = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", obj],
                         capture_output=True, text=True, check=True).stdout
    name, lines = None, []

    def close():
        if name is not None:
            out[name] = (len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16])

    for line in txt.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:\s*$", line)
        if m:
            close()
            name, lines = m.group(1), []
        elif name is not None and line.strip():
            lines.append(" ".join(line.split("//")[0].split()))
    close()


def resources(lib, hashes=False):
    """{kernel name: dict(vgpr, agpr, sgpr, vspill, sspill, scratch, lds)} for every kernel of the library's gfx950 code objects;
    hashes: also n_insn and hash, of the kernel's disassembled instructions."""
    tmp = tempfile.mkdtemp(prefix="gs_res_")
    out, code = {}, {}
    try:
        for obj in _code_objects(lib, tmp):
            _notes(obj, out)
            if hashes:
                _disassembly(obj, code)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if hashes:
        for name, r in out.items():
            r["n_insn"], r["hash"] = code.get(name, (-1, "?"))
    return out


def diff(old, new):
    """The kernels that are not the same in the two libraries, one line each; the number of such kernels."""
    a, b = resources(old, hashes=True), resources(new, hashes=True)
    n = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%-44s only in %s" % (name, new if name in b else old))
        elif a[name] != b[name]:
            what = ["%s %s -> %s" % (k, a[name][k], b[name][k]) for k in FIELDS + ("n_insn", "hash") if a[name][k] != b[name][k]]
            print("%-44s %s" % (name, ", ".join(what)))
        else:
            continue
        n += 1
    print("%d of %d kernels differ" % (n, len(set(a) | set(b))))
    return n


def main():
    args = sys.argv[1:]
    if args and args[0] == "--diff":
        if len(args) != 3:
            sys.exit(__doc__)
        sys.exit(1 if diff(args[1], args[2]) else 0)
    hashes = "--hash" in args
    args = [a for a in args if a != "--hash"]
    lib = args[0] if args and args[0].endswith(".so") else DEFAULT_LIB
    flt = args[-1] if args and not args[-1].endswith(".so") else ""
    print("%-44s %5s %5s %5s %7s %7s %8s %8s" % (("kernel",) + FIELDS) + ("  %7s %s" % ("insn", "hash") if hashes else ""))
    for name, r in sorted(resources(lib, hashes).items()):
        if flt in name:
            print("%-44s %5d %5d %5d %7d %7d %8d %8d" % ((name,) + tuple(r[k] for k in FIELDS)) + ("  %7d %s" % (r["n_insn"], r["hash"]) if hashes else ""))


if __name__ == "__main__":
    main()
