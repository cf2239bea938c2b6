#!/usr/bin/env python
"""Are two builds' gfx950 code objects the same device code?  For a host-only change: the kernels must not move.

  python tools/codeobj_diff.py DIR_A DIR_B      (each holds arcle_hip.o and arcle_big.o, compiled with the flags of arcle_amd/_lib.py)

Per unit: takes the code object out of the fat object (llvm-objdump --offloading), lists the kernel symbols (llvm-readelf --dyn-syms,
*.kd), and compares kernel by kernel the disassembly (llvm-objdump -d: mnemonics and encodings, without the addresses — the order
of the kernels in the section follows the order of instantiation in the host code and may change) and the metadata note of every
kernel (llvm-readelf --notes: VGPR / SGPR / spill counts, scratch, LDS, kernarg size and layout).  Exit status 1 on any difference."""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """llvm-objdump --offloading writes the code objects beside the file it reads: work on a copy in a directory of our own."""
    copy = shutil.copy(obj, os.path.join(tmp, os.path.basename(obj)))
    tool("llvm-objdump", "--offloading", copy)
    found = glob.glob(copy + ".*gfx950*")
    assert len(found) == 1, f"{obj}: expected one gfx950 code object, found {found}"
    return found[0]


def kernels(co):
    return sorted(line.split()[-1] for line in tool("llvm-readelf", "--dyn-syms", co).splitlines() if line.endswith(".kd"))


def functions(co):
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line.rstrip()))
    return out


def metadata(co):
    blocks = re.split(r"\n  - (?=\.agpr_count|\.args)", tool("llvm-readelf", "--notes", co))
    return {re.search(r"\.name:\s+(\S+)", b).group(1): b.split("\namdhsa.target")[0] for b in blocks[1:]}


def digest(d):
    return hashlib.sha256("\n".join(k + "\n" + (d[k] if isinstance(d[k], str) else "\n".join(d[k])) for k in sorted(d)).encode()).hexdigest()[:16]


def main(a, b):
    bad = False
    for unit in ("arcle_hip", "arcle_big"):
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            ca, cb = code_object(os.path.join(a, unit + ".o"), ta), code_object(os.path.join(b, unit + ".o"), tb)
            ka, kb, fa, fb, ma, mb = kernels(ca), kernels(cb), functions(ca), functions(cb), metadata(ca), metadata(cb)
        for k, f, m in ((ka, fa, ma), (kb, fb, mb)):  # (a parsing miss must not read as "identical")
            assert k and sorted(m) == [x[:-3] for x in k] and set(m) <= set(f), f"{unit}: {len(k)} kernels, {len(f)} functions, {len(m)} metadata entries parsed"
        dis = [k for k in set(fa) | set(fb) if fa.get(k) != fb.get(k)]
        meta = [k for k in set(ma) | set(mb) if ma.get(k) != mb.get(k)]
        print(f"{unit}: kernels {len(ka)} / {len(kb)}, same names: {'yes' if ka == kb else 'NO'}, same order: {'yes' if list(fa) == list(fb) else 'no'}; "
              f"disassembly differs for {len(dis)}, metadata for {len(meta)}; sha256 over the kernels by name: disassembly {digest(fa)} / {digest(fb)}, "
              f"metadata {digest(ma)} / {digest(mb)}")
        for k in sorted(set(ka) ^ set(kb)) + sorted(dis)[:8] + sorted(meta)[:8]:
            print("  differs:", k)
        bad = bad or ka != kb or bool(dis) or bool(meta)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
