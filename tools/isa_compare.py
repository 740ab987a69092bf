"""developer tool (CPU-only box, starts nothing on a GPU): are the gfx950 instruction streams of the kernels the same in two trees?

    python tools/isa_compare.py OLD_TREE [NEW_TREE] [--rename OLD=NEW ...] [--by-name] [--keep DIR]

Compiles every kernel unit each tree's build.py lists (the units may differ between the trees: kernels move) to device-only
assembly with that unit's flags, demangles, strips comments, directives and label numbering, pools a tree's functions by
demangled name and compares the pools.  --rename maps a name of the old tree to its name in the new one (applied to the whole
text, so a kernel's own LDS symbols follow).  --by-name pools by the name without its parameter list, for kernels whose
parameters were regrouped (their LDS symbols follow too).  NEW_TREE defaults to the tree this file is in.  Exit status 1 when a function
present in both trees differs."""
import argparse
import ast
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]


def units(tree):
    """(unit, flags) of the kernel units (*_kernels.hip) in the tree's build.py"""
    pairs = re.findall(r'\("(\w+\.hip)",\s*(\[[^\]]*\])\)', open(os.path.join(tree, "smart-chess-rust_amd", "build.py")).read())
    return [(u, ast.literal_eval(f)) for u, f in pairs if u.endswith("_kernels.hip")]


def pool(tree, tag, tmp, renames, by_name=False):
    fns = {}
    for unit, extra in units(tree):
        fns.update(functions(assembly(tree, unit, extra, os.path.join(tmp, tag + "_" + unit + ".s")), renames))
    if by_name:
        fns = {bare(n): [line.replace(n, bare(n)) for line in body] for n, body in fns.items()}
    return fns


def bare(name):
    """a demangled function name without its parameter list"""
    return re.sub(r"\(.*\)$", "", name)


def assembly(tree, unit, extra, out):
    src = os.path.join(tree, "smart-chess-rust_amd", "csrc", unit)
    subprocess.run([HIPCC] + COMMON + extra + [src, "-o", out], check=True)
    return subprocess.run(["c++filt"], stdin=open(out), stdout=subprocess.PIPE, text=True, check=True).stdout


def functions(text, renames):
    """demangled name -> normalised instruction lines"""
    for old, new in renames:
        text = re.sub(r"\b%s\b" % re.escape(old), new, text)
    fns, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(.*),@function\s*$", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\s*\.Lfunc_end\d+:", line):
            fns[name] = body
            name = None
            continue
        line = line.split(";")[0].strip()
        if not line or line.startswith(".") and not line.endswith(":") or line == name + ":":
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))   # block labels carry the function's number in the unit
    return fns


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree", nargs="?", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--by-name", action="store_true", help="pool by function name without the parameter list")
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_compare_")
    os.makedirs(tmp, exist_ok=True)
    differ = 0
    old, new = pool(a.old_tree, "old", tmp, renames, a.by_name), pool(a.new_tree, "new", tmp, [], a.by_name)
    print("== %d functions in the old tree, %d in the new" % (len(old), len(new)))
    for name in sorted(set(old) | set(new)):
        short = name if len(name) <= 110 else name[:107] + "..."
        if name not in new:
            print("  only old   %6d  %s" % (len(old[name]), short))
        elif name not in old:
            print("  only new   %6d  %s" % (len(new[name]), short))
        elif old[name] == new[name]:
            print("  identical  %6d  %s" % (len(new[name]), short))
        else:
            differ += 1
            first = next((i for i, (x, y) in enumerate(zip(old[name], new[name])) if x != y), min(len(old[name]), len(new[name])))
            print("  DIFFER     %6d -> %d (first at instruction %d)  %s" % (len(old[name]), len(new[name]), first, short))
    print("%d function(s) differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
