"""The machine code and the resource figures of named kernels in a built library, for comparing two builds without a GPU (a
refactor against its parent: a kernel whose bytes are the parent's needs no timing).

    python tools/kernel_bytes.py show-edit-tell_amd/csrc/libset_hip.so rg_score_k ed_score_k [--json out.json]

The library's .hip_fatbin section (llvm-objcopy --dump-section) holds one clang offload bundle per translation unit; the gfx950
code object of each is cut out by the bundle's own table.  A kernel is found by a substring of its mangled name; its bytes are
the symbol's range of .text (size and sha256 are printed), its registers, scratch and LDS are read from the code object's
metadata note (llvm-readelf --notes).
"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIGURES = ("sgpr_count", "vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "sgpr_spill_count",
           "vgpr_spill_count")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, stdout=subprocess.PIPE).stdout.decode()


def code_objects(fat, arch):
    """the device code objects for `arch` of every bundle in the section's bytes"""
    at = fat.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", fat, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if triple.startswith("hip") and triple.endswith(arch):
                yield fat[at + off:at + off + size]
        at = fat.find(MAGIC, at + 1)


def kernels(lib, names, arch="gfx950"):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        f = lambda n: os.path.join(tmp, n)
        tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + f("fat"), lib, f("copy"))
        for co in code_objects(open(f("fat"), "rb").read(), arch):
            open(f("co"), "wb").write(co)
            funcs = {l.split()[-1]: l.split() for l in tool("llvm-readelf", "-s", "-W", f("co")).splitlines() if " FUNC " in l}.values()
            mine = [(n, s) for n in names for s in funcs if n in s[-1]]
            if not mine:
                continue
            text = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", tool("llvm-readelf", "-S", "-W", f("co")))
            addr0, off0 = int(text.group(1), 16), int(text.group(2), 16)
            entries = tool("llvm-readelf", "--notes", f("co")).split("\n  - .agpr_count")
            for name, s in mine:
                if name in out:
                    raise SystemExit("%s: more than one function symbol holds %r" % (lib, name))
                addr, size, sym = int(s[1], 16), int(s[2]), s[-1]
                body = co[off0 + addr - addr0:off0 + addr - addr0 + size]
                meta = [".agpr_count" + e for e in entries if re.search(r"\.name:\s+%s\n" % re.escape(sym), e)]
                # self-check of the parsing: a code object (ELF), the symbol's whole range cut out of it, whole instruction
                # words, an s_endpgm (0xBF810000) among them, and exactly one metadata entry of that name with every figure
                ok = (co[:4] == b"\x7fELF" and len(body) == size > 0 and size % 4 == 0 and b"\x00\x00\x81\xbf" in body
                      and len(meta) == 1 and all(re.search(r"\.%s:\s+\d+" % fig, meta[0]) for fig in FIGURES))
                if not ok:
                    raise SystemExit("%s: cannot read %s out of the code object (has the tools' output changed?)" % (lib, sym))
                meta = meta[0]
                out[name] = {"symbol": sym, "code_bytes": size, "sha256": hashlib.sha256(body).hexdigest()}
                for fig in FIGURES:
                    out[name][fig] = int(re.search(r"\.%s:\s+(\d+)" % fig, meta).group(1))
    missing = [n for n in names if n not in out]
    if missing:
        raise SystemExit("%s: no function symbol holds %r" % (lib, missing))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("kernel", nargs="+")
    ap.add_argument("--json")
    ns = ap.parse_args()
    res = kernels(ns.lib, ns.kernel)
    for k, v in res.items():
        print(k, json.dumps(v))
    if ns.json:
        with open(ns.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
