#!/usr/bin/env python3
"""
Is the gfx950 device code of two source trees the same?  For a refactor that must not touch a kernel.

    python tools/compare_device_code.py [--diff] <tree_a> <tree_b>   (a tree: a checkout of this repository; e.g. `git worktree add`)

Every translation unit of __graft_entry__.UNITS is compiled to assembly, device side only, with the unit's own flags; the
kernels (symbols with an `amdhsa_kernel` descriptor) are compared one by one: the instruction stream from the kernel's label to
its `.Lfunc_end` (the kernel descriptor included), and the kernel's entry in the `amdgpu_metadata` note (VGPR / SGPR / AGPR counts, LDS, scratch, kernarg size,
arguments).  Local label numbers, comments and blank lines are normalised away.  Prints one line per unit and the names of the
kernels that differ or exist on one side only; exit status 0 when every kernel of every unit is identical.  A kernel whose body
differs is classified: whether the metadata entry, the number of instructions and the multiset of opcodes are the same (then only
register numbers, operand order or the order of instructions moved); --diff adds the unified diff of the two normalised bodies.
"""
import collections
import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def _entry(tree):
    spec = importlib.util.spec_from_file_location("graft_entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _asm(entry, unit, out):
    cmd = [entry.HIPCC] + entry.CXXFLAGS + entry.UNIT_FLAGS.get(unit, []) + ["--offload-device-only", "-S",
                                                                             os.path.join(entry.CSRC, unit + ".hip"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    with open(out) as f:
        return f.read()


def _normalise(lines):
    """drop comments and blank lines; number the local labels in order of first appearance"""
    names = {}
    out = []
    for ln in lines:
        ln = re.sub(r"\s*;.*$", "", ln).rstrip()
        if not ln.strip() or ln.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
            continue
        ln = re.sub(r"\.L[A-Za-z_]*\d+(_\d+)*", lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln)
        out.append(ln)
    return out


def _kernels(text):
    """{kernel name: (normalised body, normalised metadata entry)}"""
    lines = text.split("\n")
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    body = {}
    for k in names:
        a = next(i for i, ln in enumerate(lines) if ln.startswith(k + ":"))
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))     # (the kernel descriptor lies in between)
        body[k] = _normalise(lines[a + 1:b])
    meta = {}
    if "amdhsa.kernels:" in lines:
        cur = []
        for ln in lines[lines.index("amdhsa.kernels:") + 1:] + ["end"]:
            if ln.startswith("  - ") or not ln.startswith("  "):
                if cur:
                    meta[next(x.split(":", 1)[1].strip() for x in cur if x.startswith("    .name:"))] = cur
                cur = []
                if not ln.startswith("  "):
                    break
            cur.append(ln)
    return {k: (body[k], meta.get(k, [])) for k in names}


def _opcodes(body):
    """the instructions' opcodes: labels, directives and the kernel descriptor left out"""
    return [ln.split()[0] for ln in body if ln.startswith(("\t", " ")) and not ln.split()[0].startswith(".")]


def _classify(a, b):
    oa, ob = _opcodes(a[0]), _opcodes(b[0])
    return "metadata %s, %d / %d instructions, opcode multiset %s" % (
        "identical" if a[1] == b[1] else "DIFFERS", len(oa), len(ob),
        "identical" if collections.Counter(oa) == collections.Counter(ob) else "DIFFERS")


def main():
    show = "--diff" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--diff"]
    if len(args) != 2:
        sys.exit(__doc__)
    trees = [os.path.abspath(t) for t in args]
    entries = [_entry(t) for t in trees]
    units = sorted(set(entries[0].UNITS) | set(entries[1].UNITS))
    total = same = 0
    bad = []
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=6) as ex:
        jobs = {(u, i): ex.submit(_asm, entries[i], u, os.path.join(tmp, "%s_%d.s" % (u, i)))
                for u in units for i in (0, 1) if u in entries[i].UNITS}
        for u in units:
            ks = [_kernels(jobs[(u, i)].result()) if (u, i) in jobs else {} for i in (0, 1)]
            diff = [k for k in sorted(set(ks[0]) | set(ks[1])) if ks[0].get(k) != ks[1].get(k)]
            n = len(set(ks[0]) | set(ks[1]))
            total += n
            same += n - len(diff)
            print("%-12s %4d kernels, %4d identical, %d differing" % (u, n, n - len(diff), len(diff)))
            for k in diff:
                why = "only in " + trees[0 if k in ks[0] else 1] if (k in ks[0]) != (k in ks[1]) else \
                      ("body" if ks[0][k][0] != ks[1][k][0] else "metadata")
                print("    DIFFERS (%s): %s" % (why, k))
                if why == "body":
                    print("        " + _classify(ks[0][k], ks[1][k]))
                    if show:
                        print("\n".join(difflib.unified_diff(ks[0][k][0], ks[1][k][0], "a/" + k, "b/" + k, lineterm="", n=1)))
                bad.append(k)
    print("total: %d units, %d kernels, %d identical, %d differing" % (len(units), total, same, len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
