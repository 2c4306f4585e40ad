"""Hash the compiler's device listing of every source file, to show that a refactor moved no instruction.

usage: device_listing_hashes.py [--experiments] [TREE]

For every file in build.SOURCES of TREE (default: this checkout; with --experiments the -DMAL_EXPERIMENTS build, which adds
build.EXPERIMENT_SOURCES) run hipcc with that tree's build.FLAGS + --cuda-device-only -S and print the file name, the sha256 of
the listing without the lines that contain __hip_cuid_ (a per-compilation id), and the listing's line count.  Two trees whose
rows agree compile to the same kernels, register counts and LDS sizes.  Compiler warnings go to stderr."""
import concurrent.futures
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

args = sys.argv[1:]
experiments = "--experiments" in args
trees = [a for a in args if a != "--experiments"]
if len(trees) > 1 or any(a.startswith("-") for a in trees):
    sys.exit(__doc__)
tree = os.path.abspath(trees[0] if trees else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["MAL_EXPERIMENTS"] = "1" if experiments else "0"  # build.py reads it on import
spec = importlib.util.spec_from_file_location("_listing_build", os.path.join(tree, "mal_amd", "build.py"))
B = importlib.util.module_from_spec(spec)
spec.loader.exec_module(B)


def listing(src):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "listing.s")
        r = subprocess.run([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", asm],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stdout))
        with open(asm) as fh:
            text = fh.readlines()
    kept = [l for l in text if "__hip_cuid_" not in l]
    return hashlib.sha256("".join(kept).encode()).hexdigest(), len(text), r.stdout


with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
    rows = list(pool.map(listing, B.SOURCES))
width = max(len(os.path.basename(s)) for s in B.SOURCES)
for src, (digest, n, warnings) in zip(B.SOURCES, rows):
    print("%-*s  %s  %7d" % (width, os.path.basename(src), digest, n))
    if warnings.strip():
        print("%s:\n%s" % (src, warnings), file=sys.stderr)
