"""Device code of two checkouts, kernel by kernel: python scripts/isa_compare.py PARENT_ROOT BRANCH_ROOT [--jobs N] [--rename OLD=NEW ...]

Compiles every .hip under idvs/morec_amd/csrc of both trees device-only to gfx950 assembly (the command of
scripts/isa_audit.py::assembly), splits it by kernel symbol and compares, per kernel, the instruction text (basic-block labels
without the function's index in its file) and the .amdhsa_* resource lines.  Prints one line per file and exits 1 on any
difference.  --rename OLD=NEW (repeatable) replaces the substring OLD of a parent's mangled kernel symbol by NEW before the two
sides are matched; kernels are then matched over the whole library instead of file by file (a renamed kernel may have changed
files).  For every pair that differs, one line says whether the .amdhsa_* lines and the multiset of opcodes are equal.  The assembly
is kept under OUT/<label>/ (--out, default: the system's temporary directory), so a second run of an unchanged tree is instant."""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(root, src, out_dir):
    csrc = os.path.join(root, "idvs", "morec_amd", "csrc")
    out = os.path.join(out_dir, os.path.basename(src) + ".s")
    if not (os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in glob.glob(os.path.join(csrc, "*.h*")))):
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-I" + os.path.join(root, "include"), "-I" + csrc, "-S", "--cuda-device-only",
                        src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernels(lines):
    """{symbol: (instruction lines, .amdhsa_ lines)} of the kernels (symbols with a .amdhsa_kernel descriptor)."""
    body, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            t = l.split(";")[0].strip()
            if t and not t.startswith(".") or t.startswith(".LBB"):
                body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))      # .LBB<function index>_<block>: the index is the kernel's position in its file
        if l.startswith(".Lfunc_end"):
            cur = None
    res, cur = {}, None
    for l in lines:
        t = l.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = t.split()[1]
            res[cur] = []
        elif t.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and t.startswith(".amdhsa_"):
            res[cur].append(t)
    return {k: (body.get(k, []), r) for k, r in res.items()}


def describe(sym, p, b):
    """One line on a differing pair: are the resource lines equal, and which opcodes occur a different number of times."""
    ops = [collections.Counter(t.split()[0] for t in body if not t.startswith(".LBB")) for body in (p[0], b[0])]
    delta = {o: ops[1][o] - ops[0][o] for o in sorted(set(ops[0]) | set(ops[1])) if ops[0][o] != ops[1][o]}
    return (f"  {sym}: {len(p[0])} vs {len(b[0])} lines, .amdhsa_* lines {'equal' if p[1] == b[1] else 'DIFFER'}, "
            f"opcode multiset {'equal' if not delta else 'differs (branch - parent): ' + ' '.join(f'{o} {d:+d}' for o, d in delta.items())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "isa_compare"))
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]

    def renamed(sym):
        for old, new in renames:
            if old in sym:
                return sym.replace(old, new)
        return sym

    work = []
    for label, root in (("parent", a.parent), ("branch", a.branch)):
        os.makedirs(os.path.join(a.out, label), exist_ok=True)
        for src in sorted(glob.glob(os.path.join(root, "idvs", "morec_amd", "csrc", "*.hip"))):
            work.append((label, root, src))
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        asm = list(ex.map(lambda w: kernels(assembly(w[1], w[2], os.path.join(a.out, w[0]))), work))
    per = {"parent": {}, "branch": {}}
    for (label, _, src), k in zip(work, asm):
        per[label][os.path.basename(src)] = {renamed(s) if label == "parent" else s: v for s, v in k.items()}
    allp = set().union(*[set(v) for v in per["parent"].values()])
    allb = set().union(*[set(v) for v in per["branch"].values()])
    if renames:      # one pool per side: a kernel is found whichever file it sits in
        for label, files in per.items():
            pool = {}
            for f, k in files.items():
                for sym, v in k.items():
                    pool[sym + " @" + f if sym in pool else sym] = v      # a symbol that several files define: one entry per file
            per[label] = {"(whole library)": pool}
    bad = 0
    for f in sorted(set(per["parent"]) | set(per["branch"])):
        p, b = per["parent"].get(f, {}), per["branch"].get(f, {})
        diff = sorted(k for k in set(p) & set(b) if p[k] != b[k])
        only = sorted(set(p) ^ set(b))
        bad += len(diff) + len(only)
        print(f"{f}: {len(b)} kernels, {len(diff)} differ, {len(only)} only on one side" + ("" if not only else "  " + " ".join(only[:4])))
        for k in diff:
            print(describe(k, p[k], b[k]))
    print(f"library: {len(allp)} kernel symbols at the parent, {len(allb)} at the branch, symbol sets {'equal' if allp == allb else 'DIFFER'}")
    sys.exit(1 if bad or allp != allb else 0)


if __name__ == "__main__":
    main()
