#!/usr/bin/env python3
"""Per-kernel instruction streams of csrc/ files, one tree against another (CPU only).

    tools/isa_diff.py [--rev REV] [TREE_A [TREE_B]] [-o profiles/head_refactor_isa.txt]
    tools/isa_diff.py --files-a pwgemm.hip --files-b pwgemm.hip pwstream.hip pwlds.hip ... [-o profiles/pwgemm_split_isa.txt]
    tools/isa_diff.py --files-a misc.hip focal.hip --files-b misc.hip losstail.hip --rename 'xent32_kernel<false>=row_kernel<XentTerm, false, float*>' ...

Without trees, A is a temporary `git worktree` of REV (default HEAD: the parent of uncommitted work; pass HEAD~1 once
the work is committed) and B is the working tree.  Each file is cross-compiled to gfx950 device assembly with the flags
of csrc/Makefile and split per kernel.  Lines that differ between any two compiles of the same source (.file, .ident,
the __hip_cuid_* symbol) and comments are dropped, function-local label numbers are renumbered in order of appearance,
and the streams are compared as text: identical or different, with the instruction count, VGPRs, scratch and LDS bytes
of both sides.  Exit status 0 whatever the verdict: the table is the result.

Without --files-a / --files-b the output head's six files are compared file by file (one
that a tree does not have yet holds no kernels there).  With them (either one defaults to
the other) the kernels of all files of a side are pooled — code that moved between files — and paired by demangled name,
template arguments kept, `(anonymous namespace)::` and the namespace of the GEMM argument structs (`pw::`) stripped; a
kernel's own mangled symbol inside its stream is replaced by a placeholder before the comparison.  --rename OLD=NEW
(repeatable) pairs a kernel of A named OLD with the kernel of B named NEW: code whose name changed on the way.

--memseq NAME adds, below the table, for every kernel named *NAME* that both sides have: whether the sequence of
global_load_* / global_store_* instructions and vmcnt(N) waits in front of the kernel's first LDS or barrier instruction
(its main loop, in layout order) is the same on both sides, and its unified diff where it is not."""
import argparse
import concurrent.futures as cf
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

FILES = ["misc.hip", "losstail.hip", "evaltail.hip", "crfunary.hip", "mine.hip", "jaccard.hip"]
CSRC = os.path.join("keras-segmentation-deeplab-v3.1_amd", "csrc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLATILE = re.compile(r"^\s*\.(file|ident)\b|__hip_cuid_")


def make_var(text, name):
    val = os.environ.get(name) or re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1)
    return re.sub(r"\$\((\w+)\)", lambda r: make_var(text, r.group(1)), val).strip()


def compile_asm(tree, fname, out):
    if not os.path.exists(os.path.join(tree, CSRC, fname)):
        return []
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    cmd = [make_var(mk, "HIPCC")] + make_var(mk, "CXXFLAGS").split() + ["--cuda-device-only", "-S", "-o", out, fname]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.exit("%s: %s failed:\n%s" % (tree, " ".join(cmd), r.stderr))
    return open(out).read().splitlines()


def kernels(lines):
    """{mangled name: (stream, stats)} of every .amdhsa_kernel of one assembly file"""
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = lines.index(next(l for l in lines if l.startswith(name + ":")))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        labels, stream, own = {}, [], name[2:] if name.startswith("_Z") else name
        for l in lines[start + 1:end]:
            l = l.split(";")[0].rstrip()
            if not l.strip() or VOLATILE.search(l):
                continue
            l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l).replace(own, "<self>")
            stream.append(l)
        info = "\n".join(lines[end:end + 60])
        stat = lambda key: int(re.search(r"; %s:? =? ?(\d+)" % key, info).group(1))
        n_inst = sum(1 for l in stream if l.startswith("\t") and not l.lstrip().startswith("."))
        out[name] = (stream, (n_inst, stat("NumVgprs"), stat("ScratchSize"), stat("LDSByteSize")))
    return out


def mem_sequence(stream):
    """the global loads, global stores and vmcnt values in front of the first ds_* / s_barrier instruction"""
    out = []
    for l in stream:
        op = (l.split() or [""])[0]
        if op.startswith("ds_") or op == "s_barrier":
            break
        if op.startswith(("global_load", "global_store")):
            out.append(op)
        elif op == "s_waitcnt" and "vmcnt(" in l:
            out.append(re.search(r"vmcnt\(\d+\)", l).group(0))
    return out


def demangle(names):
    """{mangled name: name the kernels are paired and shown by}"""
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True)
        short = [re.sub(r"^void |\(anonymous namespace\)::|\bpw::", "", s).split("(")[0] for s in r.stdout.splitlines()]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def pool(asm, side, files, renames={}):
    """{pairing name: (file, stream, stats)} over all files of one side"""
    out = {}
    for f in files:
        pretty = {n: renames.get(p, p) for n, p in demangle(list(asm[(side, f)])).items()}
        for n, v in asm[(side, f)].items():
            if pretty[n] in out:
                sys.exit("%s: two kernels named %s (%s, %s)" % (side, pretty[n], out[pretty[n]][0], f))
            out[pretty[n]] = (f,) + v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trees", nargs="*", help="TREE_A [TREE_B]; default: a worktree of --rev, and the working tree")
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--files-a", nargs="+", metavar="FILE", help="csrc/ files of tree A, pooled (default: those of --files-b)")
    ap.add_argument("--files-b", nargs="+", metavar="FILE", help="csrc/ files of tree B, pooled (default: those of --files-a)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="with --files-a / --files-b: kernel OLD of A is paired with (and shown as) kernel NEW of B")
    ap.add_argument("-o", "--output", default=None)
    ap.add_argument("--diff", default=None, metavar="NAME", help="also print the unified diff of the kernels named *NAME*")
    ap.add_argument("--memseq", default=None, metavar="NAME",
                    help="below the table: the memory-request sequences of the kernels named *NAME*, one side against the other")
    a = ap.parse_args()
    # what is compared with what: the head's files one by one, or everything --files-a holds against everything --files-b holds
    groups = [(a.files_a or a.files_b, a.files_b or a.files_a)] if a.files_a or a.files_b else [([f], [f]) for f in FILES]
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    made = None
    if a.trees:
        ta = os.path.abspath(a.trees[0])
    else:
        ta = made = os.path.join(tmp, "parent")
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", ta, a.rev], check=True, capture_output=True)
    tb = os.path.abspath(a.trees[1]) if len(a.trees) > 1 else ROOT
    try:
        with cf.ThreadPoolExecutor(max_workers=min(10, os.cpu_count() or 1)) as ex:
            jobs = {(s, f): ex.submit(compile_asm, t, f, os.path.join(tmp, "%s_%s.s" % (s, f)))
                    for s, t, i in (("a", ta, 0), ("b", tb, 1)) for f in sorted({f for g in groups for f in g[i]})}
            asm = {k: kernels(j.result()) for k, j in jobs.items()}
    finally:
        if made:
            subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", made], capture_output=True)
        shutil.rmtree(tmp, ignore_errors=True)
    rows, n_same, n_diff = [], 0, 0
    fmt = lambda s: "%6d %5d %7d %6d" % s if s else "%6s %5s %7s %6s" % (("-",) * 4)
    n_a = n_b = 0
    diffs, both = [], []
    for fa, fb in groups:
        ka, kb = pool(asm, "a", fa, dict(r.split("=", 1) for r in a.rename)), pool(asm, "b", fb)
        n_a, n_b = n_a + len(ka), n_b + len(kb)
        for n in list(ka) + [n for n in kb if n not in ka]:
            sa, sb = ka.get(n), kb.get(n)
            verdict = "only in A" if sb is None else "only in B" if sa is None else \
                "identical" if sa[1] == sb[1] else "DIFFERENT"
            n_same += verdict == "identical"
            n_diff += verdict != "identical"
            if verdict == "DIFFERENT":
                diffs.append((n, sa[1], sb[1]))
            if sa and sb:
                both.append((n, sa[1], sb[1]))
            rows.append("%-12s %-44s %-9s | %s | %s" % ((sb or sa)[0], n, verdict, fmt(sa and sa[2]), fmt(sb and sb[2])))
    head = "%-12s %-44s %-9s | %6s %5s %7s %6s | %6s %5s %7s %6s" % (
        "file", "kernel", "stream", "A:inst", "vgpr", "scratch", "lds", "B:inst", "vgpr", "scratch", "lds")
    text = "\n".join(["# A = %s, B = %s; gfx950" % (a.trees[0] if a.trees else a.rev,
                                                    a.trees[1] if len(a.trees) > 1 else "the working tree")] +
                     ["# A's %s is B's %s" % tuple(r.split("=", 1)) for r in a.rename] + [head] + rows +
                     ["# %d kernels: %d identical, %d not; A has %d, B has %d" % (len(rows), n_same, n_diff, n_a, n_b)]) + "\n"
    for n, sa, sb in both:
        if a.memseq and a.memseq in n:
            ma, mb = mem_sequence(sa), mem_sequence(sb)
            text += "# %s: global loads / stores / vmcnt waits before the first ds_* or s_barrier: A %d, B %d, %s\n" % (
                n, len(ma), len(mb), "the same sequence" if ma == mb else "DIFFERENT sequences")
            if ma != mb:
                text += "\n".join(difflib.unified_diff(ma, mb, "A " + n, "B " + n, lineterm="", n=2)) + "\n"
    sys.stdout.write(text)
    for n, sa, sb in diffs:
        if a.diff and a.diff in n:
            sys.stdout.write("\n".join(difflib.unified_diff(sa, sb, "A " + n, "B " + n, lineterm="", n=2)) + "\n")
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
