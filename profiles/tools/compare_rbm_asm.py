"""Compare the chain kernels of two builds of rbm.hip / rbm_multi.hip from their device assembly (profiles/rbm_launch.md).

    hipcc <build.FLAGS> -S --cuda-device-only csrc/rbm.hip -o OLD/rbm.s          (likewise rbm_multi.s, and the same into NEW/)
    python profiles/tools/compare_rbm_asm.py OLD NEW

Per kernel, keyed by (single | grouped, tempered, given, form): registers, LDS, scratch and waves per SIMD of both builds, and how many
instructions differ (`diff` of the listings with register numbers and label names blanked) outside and INSIDE the k loop of the chain -- every line between a label and a backward branch to it with
a workgroup barrier in between (the set-up loops, which copy W and the rows into LDS, have none).  The last column tells a reordering from a
change: how many k-loop instructions one build has and the other has not, counted by mnemonic."""
import collections
import os
import re
import subprocess
import sys
import tempfile


def key_of(name):
    """(grouped, tempered, given, form) of a demangled chain-kernel name of either naming scheme; None for any other kernel."""
    m = re.match(r"void (rbm_gibbs_\w*kernel)<(.*)>\(", name)
    if not m:
        return None
    fn, targs = m.group(1), m.group(2)
    form = "lds" if "_lds_" in fn else "mfma" if "_mfma_" in fn else "stream"
    nums = re.findall(r"\b(\d+)\b", re.sub(r"Gibbs\w*Args<[^>]*>", "", targs))
    if form == "lds":
        form += "<%s>" % ",".join(nums[:3])
    new = re.match(r"Gibbs(Table)?Args<(\w+)>, (\w+)", targs)
    if new:
        grouped, tempered, given = new.group(1) is not None, new.group(2) == "true", new.group(3) == "true"
    else:
        grouped, tempered = "_multi_" in fn, "_temp_" in fn
        given = "unsigned char" in targs if not (grouped or tempered) else targs.split(",")[-1].strip() == "true"
    return ("grouped" if grouped else "single", "tempered" if tempered else "-", "given" if given else "-", form)


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                         r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        agpr, lds, sym, scratch, vgpr = m.groups()
        name = subprocess.check_output(["c++filt", sym], text=True).strip()
        body = text[text.index("\n" + sym + ":"):]
        body = body[:body.index("s_endpgm")].split("\n")
        seq, labels, loops = [], {}, []
        for ln in body:
            ln = ln.split(";")[0].strip()
            lab = re.match(r"(\.LBB\w+):", ln)
            if lab:
                labels[lab.group(1)] = len(seq)
            elif ln and not ln.startswith("."):
                br = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", ln)
                if br and br.group(1) in labels:
                    loops.append((labels[br.group(1)], len(seq)))
                seq.append(re.sub(r"\.LBB\w+", "L", re.sub(r"\b[sva]\[?[0-9:]+\]?", "R", ln)))
        loops = [(a, b) for a, b in loops if "s_barrier" in seq[a:b]]
        in_loop = [any(a <= i <= b for a, b in loops) for i in range(len(seq))]
        out[name] = dict(vgpr=int(vgpr), agpr=int(agpr), lds=int(lds), scratch=int(scratch), seq=seq, in_loop=in_loop)
    return out


def waves(k):
    return min(8, 512 // max(8, -(-k["vgpr"] // 8) * 8))


def main(old_dir, new_dir):
    rows = {}
    for side, d in (("old", old_dir), ("new", new_dir)):
        for f in ("rbm.s", "rbm_multi.s"):
            for name, k in kernels("%s/%s" % (d, f)).items():
                key = key_of(name) or ("other", name.split("(")[0], "", "")
                rows.setdefault(key, {})[side] = k
    print("| kernel | vgpr | agpr | lds | scratch | waves/SIMD | differing instructions outside the k loop | inside the k loop | of these, not a reordering |")
    print("|---|---|---|---|---|---|---|---|---|")
    for key in sorted(rows):
        o, n = rows[key].get("old"), rows[key].get("new")
        cell = lambda f: "%s -> %s" % (f(o) if o else "none", f(n) if n else "none")
        outside = inside = unpaired = ""
        if o and n:
            outside = inside = 0
            with tempfile.TemporaryDirectory() as tmp:
                for side, k in (("o", o), ("n", n)):
                    open(os.path.join(tmp, side), "w").write("\n".join(k["seq"]) + "\n")
                marks = subprocess.run(["diff", "--unchanged-line-format=", "--old-line-format=o %dn\n", "--new-line-format=n %dn\n",
                                        os.path.join(tmp, "o"), os.path.join(tmp, "n")], stdout=subprocess.PIPE, text=True).stdout.split("\n")
            for side, i in (ln.split() for ln in marks if ln):
                hot = (o if side == "o" else n)["in_loop"][int(i) - 1]
                inside += hot
                outside += not hot
            hist = [collections.Counter(x.split()[0] for x, hot in zip(k["seq"], k["in_loop"]) if hot) for k in (o, n)]
            unpaired = sum(((hist[0] - hist[1]) + (hist[1] - hist[0])).values())
        print("| %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (" ".join(x for x in key if x), cell(lambda k: k["vgpr"]), cell(lambda k: k["agpr"]),
                                                            cell(lambda k: k["lds"]), cell(lambda k: k["scratch"]), cell(waves), outside, inside, unpaired))
    chain = [k for k in rows if k[0] != "other"]
    print("\nchain kernels: %d before, %d after" % (sum("old" in rows[k] for k in chain), sum("new" in rows[k] for k in chain)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
