"""Device assembly of two source trees compared per kernel symbol — no GPU needed: what a refactor that must not change device
code is checked with (CHANGELOG rounds 7 and 12).
  python tools/probes/device_asm_diff.py <tree A> <tree B> [file.hip ...]      (default: every .hip of either tree's csrc)
Each file is compiled with the command of tests/test_isa_properties.py::_asm plus its tree's build.EXTRA_FLAGS.  Per kernel (a
symbol with an .amdhsa_kernel block) two things are compared: the function from its label to .Lfunc_end, with the function number
taken out of the local labels and of the loop comments that name them (it counts the functions of the file, so it moves when
the instances are emitted in another order), and the .amdhsa_kernel ... .end_amdhsa_kernel block.  A kernel
that differs is named with its register, scratch, LDS and occupancy lines from both trees.  Exit status 1 on any difference."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LOCAL = re.compile(r"(\.L(?:BB|func_begin|func_end|tmp|JTI)|Header=BB|Loop BB)\d+")   # the labels and the loop comments that name them
RESOURCES = ("NumSgprs", "NumVgprs", "NumAgprs", "TotalNumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def csrc(tree):
    return os.path.join(tree, "cmcd_amd", "csrc")


def extra_flags(tree):
    spec = importlib.util.spec_from_file_location("build_of_tree", os.path.join(tree, "cmcd_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.EXTRA_FLAGS


def asm(tree, src, flags, tmp):
    out = os.path.join(tmp, "%s_%s.s" % (abs(hash(tree)), src))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(tree, "include"), "-I", csrc(tree),
           "--cuda-device-only", "-S", "-o", out, os.path.join(csrc(tree), src), *flags.get(src, [])]
    subprocess.run(cmd, check=True, capture_output=True)
    with open(out) as fh:
        return fh.read().split("\n")


def kernels(lines):
    """-> {symbol: (body, resource block, resource comment lines)}"""
    res = {}
    for i, l in enumerate(lines):
        if not l.lstrip().startswith(".amdhsa_kernel "):
            continue
        name = l.split()[1]
        block_end = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
        start = next(k for k, m in enumerate(lines) if m.startswith(name + ":"))
        end = next(k for k in range(start + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = [LOCAL.sub(lambda m: m.group(1), m) for m in lines[start:end + 1]]
        notes = [m.strip() for m in lines[end:end + 40] if any(("; %s:" % r) in m for r in RESOURCES)]
        res[name] = (body, lines[i:block_end + 1], notes)
    return res


def sha(tree, family):
    r = subprocess.run([sys.executable, "-c", "import bench; print(bench.kernel_sources_sha(%r))" % family], cwd=tree,
                       capture_output=True, text=True, check=True)
    return r.stdout.split()[-1]


def main():
    a, b = (os.path.abspath(t) for t in sys.argv[1:3])
    files = sys.argv[3:] or sorted({f for t in (a, b) for f in os.listdir(csrc(t)) if f.endswith(".hip")})
    fa, fb = extra_flags(a), extra_flags(b)
    jobs = [(t, f, fl) for f in files for t, fl in ((a, fa), (b, fb)) if os.path.exists(os.path.join(csrc(t), f))]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=int(os.environ.get("CMCD_BUILD_JOBS", "6"))) as ex:
        out = dict(zip([(t, f) for t, f, _ in jobs], ex.map(lambda j: kernels(asm(j[0], j[1], j[2], tmp)), jobs)))
    print("A = %s\nB = %s" % (sys.argv[1], sys.argv[2]))
    for fam in ("traj", "lgcp"):
        print('bench.kernel_sources_sha("%s"): A %s, B %s' % (fam, sha(a, fam), sha(b, fam)))
    diffs, total = 0, [set(), set()]
    for f in files:
        ka, kb = out.get((a, f)), out.get((b, f))
        if ka is None or kb is None:
            print("%-20s only in %s" % (f, "B" if ka is None else "A"))
            diffs += 1
            continue
        total[0] |= set(ka)
        total[1] |= set(kb)
        changed = [k for k in sorted(set(ka) & set(kb)) if ka[k][:2] != kb[k][:2]]
        names = set(ka) == set(kb)
        diffs += len(changed) + (not names)
        print("%-20s kernels A %3d, B %3d, same names: %s, bodies and resource blocks that differ: %d"
              % (f, len(ka), len(kb), "yes" if names else "NO", len(changed)))
        for k in sorted(set(ka) ^ set(kb)):
            print("    only in %s: %s" % ("A" if k in ka else "B", k))
        for k in changed:
            print("    DIFFERENT %s (body: %s, resource block: %s)" % (k, "differs" if ka[k][0] != kb[k][0] else "equal",
                                                                    "differs" if ka[k][1] != kb[k][1] else "equal"))
            print("      A: " + " ".join(ka[k][2]))
            print("      B: " + " ".join(kb[k][2]))
    print("kernel symbols over these files: A %d, B %d, sets equal: %s" % (len(total[0]), len(total[1]),
                                                                          "yes" if total[0] == total[1] else "NO"))
    print("ALL IDENTICAL" if diffs == 0 else "DIFFERENCES: %d" % diffs)
    sys.exit(0 if diffs == 0 else 1)


if __name__ == "__main__":
    main()
