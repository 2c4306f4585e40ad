"""Build a variant of libmal_hip.so with extra compiler flags into mal_amd/lib/<name>.so (for MAL_HIP_LIB=...).
usage: build_variant.py name -DMAL_STAGE_TIMERS ...
A -DMAL_* that mal_amd.build.BUILD_SWITCHES does not list is refused: no source tests it, so the build would be the product."""
import os, re, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mal_amd import build as B
name, extra = sys.argv[1], sys.argv[2:]
for i, flag in enumerate(extra):
    m = re.match(r"-D\s*(MAL_\w*)", flag if flag != "-D" else "-D" + "".join(extra[i + 1:i + 2]))
    if m and m.group(1) not in B.BUILD_SWITCHES:
        sys.exit("build_variant.py: no source honours %s; the build-time switches are:\n%s"
                 % (m.group(1), "\n".join("  %-18s %s" % kv for kv in B.BUILD_SWITCHES.items())))
hipcc = B._hipcc()
objs = []
procs = []
tmp = os.path.join(B.LIBDIR, "_" + name)
os.makedirs(tmp, exist_ok=True)
for s in B.SOURCES:
    o = os.path.join(tmp, os.path.basename(s).replace(".hip", ".o"))
    objs.append(o)
    procs.append(subprocess.Popen([hipcc] + B.FLAGS + extra + ["-c", os.path.join(B.CSRC, s), "-o", o]))
for p in procs:
    assert p.wait() == 0
out = os.path.join(B.LIBDIR, name + ".so")
subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs, check=True)
print(out)
