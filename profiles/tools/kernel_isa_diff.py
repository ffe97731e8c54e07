#!/usr/bin/env python3
"""Is the device code of two source trees the same?  (A refactor of host code must leave every kernel as it was.)

    python profiles/tools/kernel_isa_diff.py OLD/multinn_amd/csrc NEW/multinn_amd/csrc [--work DIR] [--jobs N]

Every *.hip of both trees is compiled for the device only (hipcc ... --cuda-device-only --no-gpu-bundle-output -c: a linked gfx950
ELF without relocations), with the flags multinn_amd/build.py gives that source.  Per function symbol -- the union over all objects
of a tree; a kernel that several translation units instantiate must be the same in all of them -- the disassembly is compared with
addresses and encodings stripped (branch targets are relative), and per kernel the metadata fields FIELDS.  Whole texts are
compared: no instruction is looked for.  Exit status 0 only when both trees have the same symbols and every one is identical.

A directory that holds *.co files and no *.hip is taken as already compiled objects (a kept --work/a or --work/b).
"""
import argparse
import concurrent.futures
import difflib
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def flags_for(csrc, src):
    """The flags of the tree's own build.py (beside csrc/), so that a tree is compiled the way it builds itself."""
    path = os.path.join(csrc, "..", "build.py")
    if not os.path.exists(path):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "multinn_amd", "build.py")
    spec = importlib.util.spec_from_file_location("mnn_build_" + str(abs(hash(os.path.abspath(path)))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.flags_for(src))


def compile_tree(csrc, out, jobs):
    if not glob.glob(os.path.join(csrc, "*.hip")) and glob.glob(os.path.join(csrc, "*.co")):
        return sorted(glob.glob(os.path.join(csrc, "*.co")))
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmds = []
    for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        obj = os.path.join(out, os.path.basename(src)[:-4] + ".co")
        cmds.append((obj, [hipcc] + flags_for(csrc, src) + ["--cuda-device-only", "--no-gpu-bundle-output", "-w", "-c", src, "-o", obj]))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for (obj, cmd), rc in zip(cmds, pool.map(lambda c: subprocess.call(c[1]), cmds)):
            if rc != 0:
                sys.exit("hipcc failed: " + " ".join(cmd))
    return [obj for obj, _ in cmds]


def disassembly(obj):
    """{symbol: text}: one instruction per line, without the address / encoding comment."""
    out = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", obj], text=True)
    syms, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    for s in syms:                       # the padding between two functions is not the function's
        while syms[s] and syms[s][-1] in ("s_nop 0", "s_code_end", "..."):
            syms[s].pop()
    return {s: "\n".join(t) for s, t in syms.items()}


def metadata(obj):
    """{kernel: {field: value}} from the AMDGPU metadata note."""
    out = subprocess.check_output([os.path.join(LLVM, "llvm-readelf", ), "--notes", obj], text=True)
    kernels, cur = {}, None
    for line in out.splitlines():
        if line.startswith("  - "):       # a new entry of amdhsa.kernels (argument entries are indented deeper)
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.[a-z_]+):\s*(\S.*)?$", line)
        if cur is None or not m:
            if not line.startswith(" "):
                cur = None
            continue
        if m.group(1) == ".name":
            kernels[m.group(2)] = cur
        elif m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return kernels


def tree_view(objs):
    """symbol -> set of (disassembly, metadata) over the objects that hold it"""
    view = {}
    for obj in objs:
        dis, meta = disassembly(obj), metadata(obj)
        missing = [k for k in meta if k not in dis]
        if missing:
            sys.exit(f"{obj}: kernels without code: {missing}")
        for sym, text in dis.items():
            view.setdefault(sym, {})[(text, tuple(sorted(meta.get(sym, {}).items())))] = os.path.basename(obj)
    return view


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--work", default=None, help="directory for the code objects (kept); default: a temporary one")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--show", type=int, default=40, help="diff lines printed per differing symbol")
    a = ap.parse_args()
    tmp = None
    if a.work is None:
        tmp = tempfile.TemporaryDirectory()
        a.work = tmp.name
    old = tree_view(compile_tree(a.old, os.path.join(a.work, "a"), a.jobs))
    new = tree_view(compile_tree(a.new, os.path.join(a.work, "b"), a.jobs))
    kernels_old = {s for s, v in old.items() if any(m for _, m in v)}
    kernels_new = {s for s, v in new.items() if any(m for _, m in v)}
    bad = 0
    for s in sorted(set(old) - set(new)):
        print("only in old:", s)
        bad += 1
    for s in sorted(set(new) - set(old)):
        print("only in new:", s)
        bad += 1
    same = same_kernels = 0
    for s in sorted(set(old) & set(new)):
        if set(old[s]) == set(new[s]) and len(old[s]) == 1:
            same += 1
            same_kernels += s in kernels_old
            continue
        bad += 1
        print(f"DIFFERS: {s}  (old: {sorted(old[s].values())}, new: {sorted(new[s].values())})")
        (to, mo), (tn, mn) = sorted(old[s])[0], sorted(new[s])[0]
        if mo != mn:
            print("  metadata old", dict(mo), "new", dict(mn))
        for i, line in enumerate(difflib.unified_diff(to.splitlines(), tn.splitlines(), "old", "new", lineterm="", n=1)):
            if i >= a.show:
                print("  ...")
                break
            print("  " + line)
    objs = lambda v: len({o for e in v.values() for o in e.values()})
    print(f"objects: old {objs(old)}, new {objs(new)}")
    print(f"kernels: old {len(kernels_old)}, new {len(kernels_new)}; compared {len(kernels_old & kernels_new)}, identical {same_kernels}")
    print(f"function symbols (kernels included): compared {len(set(old) & set(new))}, identical {same}")
    print("RESULT:", "identical device code" if bad == 0 and kernels_old == kernels_new else f"{bad} differences")
    return 0 if bad == 0 and kernels_old == kernels_new else 1


if __name__ == "__main__":
    sys.exit(main())
