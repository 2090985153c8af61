#!/usr/bin/env python3
"""tools/isa_diff.py OLD_TREE NEW_TREE [--flags=-DGK_PROF]: compare the gfx950
device code of two trees' sketches-py_amd/csrc/*.hip, function by function.

Each tree compiles with its own Makefile's HIPFLAGS (no GPU needed); functions
pair by mangled name, whichever unit holds them.  Compared: the bodies without
comments, trailing blanks and the function index of local labels, and the
kernel-resource-usage remarks; nothing else.  Exit 1 on any difference or on a
name that two units of one tree define."""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile


def compile_tree(root, extra=()):
    """{unit: (device assembly, {function: {remark: value}})} of a tree's csrc."""
    csrc = os.path.join(root, "sketches-py_amd", "csrc")
    flags = subprocess.run(["make", "-s", "--eval", "isa-flags:;@echo $(HIPCC) $(HIPFLAGS)", "isa-flags"], cwd=csrc,
                           capture_output=True, text=True, check=True).stdout.split() + list(extra)

    def one(hip):
        out = os.path.join(tmp, os.path.basename(hip) + ".s")
        cmd = flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", hip, "-o", out]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s\n%s" % (" ".join(cmd), r.stderr[-3000:]))
        res, cur = {}, None
        for m in re.finditer(r"remark:\s+(.+?): (\S+) \[-Rpass", r.stderr):
            if m.group(1) == "Function Name":
                cur = res.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = m.group(2)
        return os.path.basename(hip), (open(out).read(), res)

    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(16) as ex:
        return dict(ex.map(one, sorted(glob.glob(csrc + "/*.hip"))))


def functions(text):
    """{mangled name: normalised body lines} of one unit's assembly."""
    funcs = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n", text, re.M):
        body = text[text.index("\n%s:" % m.group(1), m.end() - 1):text.index("\n.Lfunc_end", m.end())]
        lines = (re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0]).rstrip() for l in body.splitlines()[2:])
        funcs[m.group(1)] = [l for l in lines if l]
    return funcs


def tree(root, extra=()):
    """(bodies, remarks, unit of each function, names that two units define)."""
    funcs, res, where, twice = {}, {}, {}, []
    for unit, (text, r) in compile_tree(root, extra).items():
        f = functions(text)
        twice += ["%s: in %s and %s" % (n, where[n], unit) for n in f if n in where]
        where.update((n, unit) for n in f)
        funcs.update(f)
        res.update(r)
    return funcs, res, where, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--flags", default="", help="extra compile flags for both trees")
    a = ap.parse_args()
    (fo, ro, wo, to), (fn, rn, wn, tn) = tree(a.old, a.flags.split()), tree(a.new, a.flags.split())
    out = ["TWICE (old)  " + t for t in to] + ["TWICE (new)  " + t for t in tn]
    for n in sorted(set(fo) | set(fn)):
        if n not in fo or n not in fn:
            out.append("ONLY %s  %s (%s)" % ("new" if n in fn else "old", n, (wn if n in fn else wo)[n]))
            continue
        if fo[n] != fn[n]:
            k = next((i for i, (x, y) in enumerate(zip(fo[n], fn[n])) if x != y), min(len(fo[n]), len(fn[n])))
            out.append("DIFF  %s (%s -> %s), from line %d:\n%s" % (n, wo[n], wn[n], k, "\n".join(
                "   - %s\n   + %s" % ("".join(fo[n][i:i + 1]), "".join(fn[n][i:i + 1])) for i in range(k, k + 4))))
        if ro.get(n) != rn.get(n):
            out.append("RESOURCES  %s\n   - %s\n   + %s" % (n, ro.get(n), rn.get(n)))
    for side, f, w in (("old", fo, wo), ("new", fn, wn)):
        print("%s: %d functions (%s)" % (side, len(f), ", ".join(
            "%s %d" % (u, list(w.values()).count(u)) for u in sorted(set(w.values())))))
    print("\n".join(out + ["%d common, %d with remarks, %d findings" % (len(set(fo) & set(fn)), len(set(ro) & set(rn)), len(out))]))
    return 1 if out else 0


if __name__ == "__main__":
    sys.exit(main())
