#!/usr/bin/env python3
"""Did a refactor leave the kernels' machine code alone?  (hipcc only, no GPU.)

    python tools/isa_same.py <other-tree> [--renamed 'OLD=NEW']... [--removed NAME]...

Every .hip source of this tree and of <other-tree> (a checkout of the commit to compare against) is compiled to gfx950
assembly with the library's flags (build.py's FLAGS, `--cuda-device-only -S`), and the kernels are compared one by one,
keyed by mangled name:
  * the instruction lines between the kernel's label and its end, without comments, blank lines and `.loc` / `.cfi`
    lines, the function index taken out of local labels (`.LBB<k>_<m>`, `.Lfunc_begin<k>` / `.Lfunc_end<k>`: it counts
    the functions of the FILE, so it moves when a kernel changes files);
  * every `.amdhsa_*` line of its kernel descriptor: registers, LDS, scratch, kernel-argument size, enabled inputs.
OLD / NEW / NAME are demangled names without the namespace and the parameter list (`k_name<true, 3>`): a kernel of
<other-tree> called OLD is compared with this tree's NEW (a rename changes the mangled name), one called NAME may be
missing here.  Any other kernel missing on either side, and any difference, is reported; the exit status is then 1."""
import difflib
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "gpu-lossless-compression_amd"
def flags():
    spec = importlib.util.spec_from_file_location("glc_build", os.path.join(ROOT, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FLAGS, os.environ.get("HIPCC", os.path.join(mod.rocm_root(), "bin", "hipcc"))


def normal(line):
    line = line.split(";")[0].rstrip()
    if not line.strip() or re.match(r"\s*\.(loc|cfi_\w+)\b", line):
        return None
    line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line)
    return re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)


def kernels_of(asm):
    """{mangled name: (instruction lines, descriptor lines)} of one file's assembly.  A kernel's text runs from its label to
    its `.Lfunc_end`; the descriptor sits inside, behind the code, from `.amdhsa_kernel` to `.end_amdhsa_kernel`."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur, part = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur, part = m.group(1), "code"
            out[cur] = ([], [])
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"\s*\.amdhsa_kernel\b", line):
            part = "descriptor"
            while out[cur][0] and re.match(r"\s*\.(section|p2align)\b", out[cur][0][-1]):
                out[cur][0].pop()                              # the descriptor's own section and alignment
        elif cur and line.strip() == ".end_amdhsa_kernel":
            part = None
        elif cur and part == "code":
            n = normal(line)
            if n is not None:
                out[cur][0].append(n)
        elif cur and part == "descriptor" and line.split()[0].startswith(".amdhsa_"):
            out[cur][1].append(" ".join(line.split()))
    return out


def tree_kernels(tree, fl, hipcc):
    csrc = os.path.join(tree, PKG, "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def cc(f):
        r = subprocess.run([hipcc] + fl + ["--cuda-device-only", "-S", "-o", "-", os.path.join(csrc, f)], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("hipcc failed on %s\n%s" % (os.path.join(csrc, f), r.stderr[-2000:]))
        return kernels_of(r.stdout)

    out = {}
    with ThreadPoolExecutor(max_workers=8) as ex:
        for f, ks in zip(files, ex.map(cc, files)):
            for k, v in ks.items():
                out[k] = v + (f,)
    return out


def short_names(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return {n: re.sub(r"^(void )?glc::", "", d).split("(")[0] for n, d in zip(names, r.stdout.splitlines())}


def main():
    args, renamed, removed = sys.argv[1:], {}, set()
    other = None
    while args:
        a = args.pop(0)
        if a == "--renamed":
            old, new = args.pop(0).split("=")
            renamed[old] = new
        elif a == "--removed":
            removed.add(args.pop(0))
        else:
            other = a
    if not other:
        raise SystemExit(__doc__)
    fl, hipcc = flags()
    here, there = tree_kernels(ROOT, fl, hipcc), tree_kernels(os.path.abspath(other), fl, hipcc)
    sh_here, sh_there = short_names(sorted(here)), short_names(sorted(there))
    by_short = {}
    for n in here:
        by_short.setdefault(sh_here[n], []).append(n)
    bad = same = 0
    matched = set()
    for n in sorted(there):
        s = sh_there[n]
        if s in renamed:
            cand = by_short.get(renamed[s], [])
            m = cand[0] if len(cand) == 1 else None
        else:
            m = n if n in here else None
        if m is None:
            if s in removed:
                print("removed   %s (%s)" % (s, there[n][2]))
            else:
                print("MISSING   %s (%s): in %s only" % (s, there[n][2], other))
                bad += 1
            continue
        matched.add(m)
        diffs = [w for w, a, b in (("instructions", there[n][0], here[m][0]), ("descriptor", there[n][1], here[m][1])) if a != b]
        if diffs:
            bad += 1
            print("DIFFERENT %s (%s -> %s): %s" % (sh_here[m], there[n][2], here[m][2], ", ".join(diffs)))
            for w, a, b in (("instructions", there[n][0], here[m][0]), ("descriptor", there[n][1], here[m][1])):
                for d in list(difflib.unified_diff(a, b, "other", "this", lineterm="", n=0))[:40]:
                    print("    " + d)
        else:
            same += 1
            if s in renamed or there[n][2] != here[m][2]:
                print("same      %s (%s) = %s (%s), %d instruction lines" % (s, there[n][2], sh_here[m], here[m][2], len(here[m][0])))
    for n in sorted(set(here) - matched):
        print("NEW       %s (%s): in this tree only" % (sh_here[n], here[n][2]))
        bad += 1
    print("kernels: %d in %s, %d here; %d compared equal, %d differences or unexpected" % (len(there), other, len(here), same, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
