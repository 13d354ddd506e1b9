"""Compare the gfx950 ISA of two source trees, kernel by kernel (cross-compiles: no GPU needed).

    python tools/isa_diff.py TREE_A TREE_B

Every .hip of build.SOURCES is compiled in both trees with the product flags (build.HIP_FLAGS + build.EXTRA_FLAGS) to assembly.
One line per kernel: `same`, `only in A`, `only in B`, or `differs` with the first differing line (instructions, the kernel
descriptor, and the register / LDS / scratch / spill numbers of the metadata).  Exit status 1 on any `differs` or `only in B`:
a refactor of B = A may drop kernels nothing launches, and nothing else."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from specforge_amd import build  # noqa: E402

# kernels that lost a template parameter between A and B: (pattern on A's demangled name, replacement)
RENAMED = [(r"(gemm_nt_256w4_kernel<\d+, \d+, \d+), 0>", r"\1>")]      # ABL (always 0)
CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count")


def compile_unit(job):
    tree, src, out = job
    csrc = os.path.join(tree, "specforge_amd", "csrc")
    flags = [csrc if f == build.CSRC else f for f in build.HIP_FLAGS] + build.EXTRA_FLAGS.get(src, [])
    subprocess.run([build.HIPCC] + flags + ["-w", "-S", "--cuda-device-only", "-o", out, os.path.join(csrc, src)], check=True)


def kernels(path):
    """{demangled name: normalised lines} of one assembly file"""
    txt = open(path).read()
    lines = txt.split("\n")
    names = re.findall(r"^\t\.amdhsa_kernel (\S+)$", txt, re.M)
    plain = subprocess.run([CXXFILT], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    res = {}
    for sym, name in zip(names, plain):
        i = lines.index(next(l for l in lines if l.startswith(sym + ":")))
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = []
        for l in lines[i + 1:j]:
            l = re.sub(r"\s*;.*$", "", l).replace(sym, "<kernel>").rstrip()
            l = re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", l)          # (labels carry the function's index in its file)
            if l.strip() and not re.match(r"\s*\.(file|ident)\b", l):
                body.append(l)
        meta = re.search(r"\.name:\s+%s\n(?:.*\n)*?.*\.wavefront_size" % re.escape(sym), txt)
        block = txt[txt.rfind("\n  - ", 0, meta.start()):meta.end()]
        for k in META:
            body.append("%s %s" % (k, re.search(r"\.%s:\s+(\d+)" % k, block).group(1)))
        res[name] = body
    return res


def main():
    tree_a, tree_b = (os.path.abspath(t) for t in sys.argv[1:3])
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for tag, tree in (("A", tree_a), ("B", tree_b)):
            os.makedirs(os.path.join(tmp, tag))
            jobs += [(tree, s, os.path.join(tmp, tag, s.replace(".hip", ".s"))) for s in build.SOURCES
                     if os.path.exists(os.path.join(tree, "specforge_amd", "csrc", s))]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
            list(ex.map(compile_unit, jobs))
        bad = 0
        for s in build.SOURCES:
            ka, kb = ({} if not os.path.exists(p) else kernels(p) for p in (os.path.join(tmp, t, s.replace(".hip", ".s")) for t in "AB"))
            for pat, rep in RENAMED:
                ka = {re.sub(pat, rep, n): v for n, v in ka.items()}
            for n in sorted(set(ka) | set(kb)):
                if n not in kb:
                    verdict = "only in A"
                elif n not in ka:
                    verdict = "only in B"
                elif ka[n] == kb[n]:
                    verdict = "same (%d lines)" % len(ka[n])
                else:
                    d = next((i for i, (x, y) in enumerate(zip(ka[n], kb[n])) if x != y), min(len(ka[n]), len(kb[n])))
                    verdict = "differs at line %d: A `%s` B `%s`" % (d, "".join(ka[n][d:d + 1]).strip(), "".join(kb[n][d:d + 1]).strip())
                bad += verdict.startswith(("differs", "only in B"))
                print("%-22s %-60s %s" % (s, n[:200].replace("(anonymous namespace)::", ""), verdict))
        print("%s" % ("FAIL: %d kernels differ or are new" % bad if bad else "OK: no kernel of B differs from A's"))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
