#!/usr/bin/env python3
"""Are two source trees' GPU kernels the same machine code?

    python scripts/kernel_identity.py <parent tree> <this tree> [--out FILE] [--jobs N]

For each tree, every meta-gcn_amd/csrc/*.hip is compiled for the device alone
(the Makefile's FLAGS, the per-file extra flags of its `build/<name>.o: FLAGS +=`
lines, --cuda-device-only), the gfx950 code object is taken out of the offload
bundle, and every kernel symbol (a function with a `<name>.kd` descriptor) gets
three sha256 digests: its machine-code bytes, its kernel descriptor (without
the code-entry offset, which is the distance between the two in the object)
and its entry in the `llvm-readelf --notes` metadata.  The kernels of a tree
are the union over its files, so a kernel may move between files.  Builds:
the product, the experiment build (-DMGCN_EXPERIMENT=1; the kernels named in
EXPERIMENT_DIFFER write the tail timers, device globals, and may differ) and
-DMGCN_XW_PROFILE (this tree only: it must compile).  Needs no GPU.  The
script hashes and compares; it looks at no instruction.
"""
import argparse
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

TARGET = "hip-amdgcn-amd-amdhsa--gfx950"
# experiment build: kernels that address the tail-timer device globals
EXPERIMENT_DIFFER = ("spmm_xw_fwd_kernel", "spmm_xw_bwd_ws_kernel")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1).strip()
    hipcc = os.environ.get("HIPCC", var("HIPCC"))
    flags = var("FLAGS").replace("$(ARCH)", var("ARCH")).split()
    extra = {m.group(1): m.group(2).split()
             for m in re.finditer(r"^build/(\w+)\.o:\s*FLAGS\s*\+=\s*(.*)$", text, re.M)}
    return hipcc, flags, extra


def llvm_tool(hipcc, name):
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for d in ("llvm/bin", "lib/llvm/bin", "bin"):
        p = os.path.join(rocm, d, name)
        if os.path.exists(p):
            return p
    return name


def code_object(tree, src, defines, tmp, tag):
    """Compile one file for the device; returns the gfx950 ELF's bytes."""
    csrc = os.path.join(tree, "meta-gcn_amd", "csrc")
    hipcc, flags, extra = makefile_flags(csrc)
    stem = src[:-4]
    out = os.path.join(tmp, "%s_%s.o" % (tag, stem))
    cmd = [hipcc] + flags + extra.get(stem, []) + defines + [
        "-I" + os.path.join(tree, "include"), "--cuda-device-only", "-c", src, "-o", out]
    subprocess.run(cmd, cwd=csrc, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    elf = out
    if open(out, "rb").read(24) == b"__CLANG_OFFLOAD_BUNDLE__":
        elf = out + ".elf"
        subprocess.run([llvm_tool(hipcc, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=" + TARGET, "--input=" + out, "--output=" + elf], check=True)
    notes = subprocess.run([llvm_tool(hipcc, "llvm-readelf"), "--notes", elf], check=True,
                           capture_output=True, text=True).stdout
    return open(elf, "rb").read(), notes


def elf_symbols(data):
    """ELF64 little-endian: {name: bytes of the symbol}."""
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, "not a 64-bit LE ELF"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for sec in secs:
        if sec[1] != 2:  # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for off in range(sec[4], sec[4] + sec[5], sec[9]):
            name_i, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", data, off)
            if shndx == 0 or shndx >= shnum or size == 0:
                continue
            end = data.index(b"\0", stroff + name_i)
            name = data[stroff + name_i:end].decode()
            s = secs[shndx]
            if s[1] == 8:  # SHT_NOBITS
                continue
            start = s[4] + (value - s[3])
            out[name] = data[start:start + size]
    return out


def metadata_entries(notes):
    """{kernel symbol: text of its amdhsa.kernels entry}."""
    out = {}
    m = re.search(r"^(\s*)amdhsa\.kernels:\s*$", notes, re.M)
    if not m:
        return out
    body = notes[m.end():]
    item = re.compile(r"^%s\s*- " % m.group(1), re.M)
    starts = [x.start() for x in item.finditer(body)]
    stop = re.search(r"^%s[\w.]" % m.group(1), body, re.M)
    limit = stop.start() if stop else len(body)
    starts = [s for s in starts if s < limit]
    for a, b in zip(starts, starts[1:] + [limit]):
        entry = body[a:b]
        sym = re.search(r"\.symbol:\s*'?\"?([^\s'\"]+?)\.kd", entry)
        if sym:
            out[sym.group(1)] = entry
    return out


def file_kernels(tree, src, defines, tmp, tag):
    data, notes = code_object(tree, src, defines, tmp, tag)
    syms = elf_symbols(data)
    meta = metadata_entries(notes)
    out = {}
    for name, kd in syms.items():
        if not name.endswith(".kd"):
            continue
        k = name[:-3]
        kd = kd[:16] + b"\0" * 8 + kd[24:]  # kernel_code_entry_byte_offset: layout, not code
        out[k] = {"code_sha256": sha(syms[k]), "kd_sha256": sha(kd),
                  "metadata_sha256": sha(meta[k].encode())}
    return out


def tree_kernels(tree, defines, tmp, tag, jobs):
    csrc = os.path.join(tree, "meta-gcn_amd", "csrc")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(jobs) as ex:
        per = list(ex.map(lambda f: file_kernels(tree, f, defines, tmp, tag), srcs))
    return dict(zip(srcs, per))


def compare(parent, tree, may_differ=()):
    """Kernels keyed by symbol (a symbol defined in several files: one record per file)."""
    def index(files):
        out = {}
        for f, ks in files.items():
            for k, h in ks.items():
                out.setdefault(k, []).append((f, h))
        return out
    a, b = index(parent), index(tree)
    digests = lambda v: sorted(json.dumps(h, sort_keys=True) for _, h in v)
    res = {"kernels_parent": sum(len(v) for v in a.values()),
           "kernels_tree": sum(len(v) for v in b.values()),
           "missing": sorted(set(a) - set(b)), "new": sorted(set(b) - set(a)),
           "differing": [], "allowed_to_differ": {}, "moved": {}}
    same = []
    for k in sorted(set(a) & set(b)):
        if digests(a[k]) == digests(b[k]):
            same.append((k, digests(b[k])))
        else:
            allowed = [n for n in may_differ if n in k]
            if allowed:  # counted per kernel template
                res["allowed_to_differ"][allowed[0]] = res["allowed_to_differ"].get(allowed[0], 0) + 1
            else:
                res["differing"].append(k)
        fa, fb = sorted(f for f, _ in a[k]), sorted(f for f, _ in b[k])
        if fa != fb:  # instantiations that changed file, counted per (from -> to)
            key = "%s -> %s" % (",".join(fa), ",".join(fb))
            res["moved"][key] = res["moved"].get(key, 0) + 1
    # one digest over every equal kernel's name and three digests
    res["equal_kernels"] = len(same)
    res["equal_kernels_sha256"] = sha(json.dumps(same).encode())
    res["files"] = {}
    for f in sorted(set(parent) | set(tree)):
        n = (len(parent.get(f, {})), len(tree.get(f, {})))
        if n != (0, 0):
            res["files"][f] = {"kernels_parent": n[0], "kernels_tree": n[1]}
    res["identical"] = not (res["missing"] or res["new"] or res["differing"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    parent, tree = os.path.abspath(args.parent), os.path.abspath(args.tree)
    result = {"how": " ".join(__doc__.split("\n\n", 2)[2].split())}
    with tempfile.TemporaryDirectory() as tmp:
        for build, defines in (("product", []), ("experiment", ["-DMGCN_EXPERIMENT=1"])):
            p = tree_kernels(parent, defines, tmp, "p_" + build, args.jobs)
            t = tree_kernels(tree, defines, tmp, "t_" + build, args.jobs)
            result[build] = compare(p, t, EXPERIMENT_DIFFER if defines else ())
            print("%s: %d kernels, identical: %s" % (build, result[build]["kernels_tree"],
                                                    result[build]["identical"]), flush=True)
        prof = tree_kernels(tree, ["-DMGCN_XW_PROFILE"], tmp, "t_prof", args.jobs)
        result["xw_profile"] = {"compiles": True, "kernels": sum(len(v) for v in prof.values())}
    result["all_kernels_identical"] = result["product"]["identical"] and result["experiment"]["identical"]
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
    else:
        print(text)
    return 0 if result["all_kernels_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
