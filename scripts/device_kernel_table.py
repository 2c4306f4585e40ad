"""Per-kernel resource table of two trees, for the source files whose device listing a refactor was expected to move.

usage: device_kernel_table.py PARENT_TREE BRANCH_TREE FILE.hip [FILE.hip ...]

For each FILE (a name from build.SOURCES) compile both trees' copy as scripts/device_listing_hashes.py does (that tree's
build.FLAGS + --cuda-device-only -S) and print, per kernel: VGPR (AGPRs included) / SGPR / LDS bytes / scratch bytes from the listing's
metadata and the instruction count between the kernel's label and its s_endpgm, parent against branch.  A row is marked NO when
LDS or scratch grew or the VGPR count crossed into a lower waves-per-SIMD tier (512 registers per SIMD lane in units of 8:
<= 64 -> 8 waves, <= 72 -> 7, <= 80 -> 6, <= 96 -> 5, <= 128 -> 4, <= 168 -> 3, <= 256 -> 2, above -> 1); a kernel with
more instructions than the parent's is listed below the table, and the opcode histogram's difference follows."""
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

if len(sys.argv) < 4:
    sys.exit(__doc__)
os.environ.setdefault("MAL_EXPERIMENTS", "0")


def build_of(tree):
    spec = importlib.util.spec_from_file_location("_table_build_%d" % abs(hash(tree)), os.path.join(tree, "mal_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(B, src):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "listing.s")
        subprocess.run([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", asm], check=True,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return open(asm).read()


def demangle(names):
    out = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"\(.*\)$", "", d).replace("void ", "").replace("mal::", "") for n, d in zip(names, out)}


def waves(vgpr):
    for limit, n in ((64, 8), (72, 7), (80, 6), (96, 5), (128, 4), (168, 3), (256, 2)):
        if vgpr <= limit:
            return n
    return 1


def kernels(text):
    """{mangled name: (vgpr, sgpr, lds, scratch, instructions, opcode Counter)}"""
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        # .vgpr_count is the unified register file's: the AGPRs are in it
        meta[name] = (get("vgpr_count"), get("sgpr_count"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    lines = text.split("\n")
    out = {}
    for name, m in meta.items():
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        ops = collections.Counter()
        for l in lines[start + 1:]:
            t = l.strip()
            if not t or t.startswith((";", ".")) or t.endswith(":"):
                continue
            ops[t.split()[0]] += 1
            if t.startswith("s_endpgm"):
                break
        out[name] = m + (sum(ops.values()), ops)
    return out


parent, branch = build_of(os.path.abspath(sys.argv[1])), build_of(os.path.abspath(sys.argv[2]))
for src in sys.argv[3:]:
    kp, kb = kernels(listing(parent, src)), kernels(listing(branch, src))
    names = demangle(sorted(set(kp) | set(kb)))
    print("  %s" % src)
    print("  %-58s %-24s %-24s %s" % ("kernel", "parent v/s/lds/scr/ins", "branch v/s/lds/scr/ins", "ok"))
    more, hist = [], collections.Counter()
    for n in sorted(names, key=names.get):
        a, b = kp.get(n), kb.get(n)
        fmt = lambda k: "%d/%d/%d/%d/%d" % k[:5] if k else "-"
        ok = bool(a and b) and b[2] <= a[2] and b[3] <= a[3] and waves(b[0]) >= waves(a[0])
        print("  %-58s %-24s %-24s %s" % (names[n][:58], fmt(a), fmt(b), "yes" if ok else "NO"))
        if a and b:
            if b[4] > a[4]:
                more.append("%s +%d" % (names[n], b[4] - a[4]))
            hist.update(b[5])
            hist.subtract(a[5])
    print("  total instructions: parent %d, branch %d" % (sum(k[4] for k in kp.values()), sum(k[4] for k in kb.values())))
    print("  more instructions than the parent's: %s" % (", ".join(more) or "none"))
    print("  opcode histogram, branch - parent: %s" % (", ".join("%s %+d" % (o, d) for o, d in sorted(hist.items()) if d) or "equal"))
