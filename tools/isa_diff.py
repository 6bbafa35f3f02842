"""Same machine code? Compiles the head units of two checkouts for gfx950 (no GPU needed) and compares every kernel: the instruction
text (comments stripped, local labels renumbered in order of appearance) and the resource fields of its descriptor (VGPRs, AGPRs, SGPRs,
LDS bytes, private segment size, spill counts). One line per kernel; exit status 1 on any difference or on a kernel that only one side
has. What a refactor that only moves kernel text between files and units must show (DESIGN_HISTORY.md, the head unit's split).

    python tools/isa_diff.py OLD_CHECKOUT NEW_CHECKOUT [--diag] [--prefix head_]
"""
import argparse
import importlib.util
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_scan import compile_units  # noqa: E402

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def build_module(checkout):
    spec = importlib.util.spec_from_file_location("acez_build_" + re.sub(r"\W", "_", checkout), os.path.join(checkout, "acezero_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels(path):
    """{symbol: (normalised instruction text, resource fields)} of one .s file"""
    text = open(path).read()
    res = {}
    for chunk in re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")])[1:]:
        name = re.search(r"\.name:\s+(\S+)", chunk).group(1)
        res[name] = tuple(int(re.search(r"\%s:\s+(\d+)" % f, chunk).group(1)) for f in FIELDS)
    out = {}
    for name, fields in res.items():
        body = text[text.index("\n%s:" % name):]
        body = body[:re.search(r"\n\.Lfunc_end\d+:", body).start()].split("\n")[2:]
        labels = {}
        lines = []
        for ln in body:
            ln = ln.split(";")[0].strip()
            if ln:
                lines.append(re.sub(r"\.L[A-Za-z_]+\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln))
        out[name] = ("\n".join(lines), fields)
    return out


def side(checkout, diag, prefix, out):
    found = {}
    for s in compile_units(build_module(checkout), out, prefix, ["-DACEZ_DIAG"] if diag else []):
        for name, k in kernels(s).items():
            found[name] = (os.path.basename(s).split("-hip-")[0],) + k
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--diag", action="store_true", help="the diagnostics build (-DACEZ_DIAG)")
    ap.add_argument("--prefix", default="head_", help="units to compare, by name prefix")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t:
        old, new = (side(os.path.abspath(c), a.diag, a.prefix, os.path.join(t, d)) for c, d in ((a.old, "old"), (a.new, "new")))
    same = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if o and n and o[1:] == n[1:]:
            verdict = "identical"
            same += 1
        elif o and n:
            verdict = "DIFFERS:" + (" code %d -> %d lines" % (o[1].count("\n") + 1, n[1].count("\n") + 1) if o[1] != n[1] else "")
            verdict += "".join(" %s %d -> %d" % (f, x, y) for f, x, y in zip(FIELDS, o[2], n[2]) if x != y)
        else:
            verdict = "ONLY IN " + ("old" if o else "new")
        print("%-12s %-12s %-100s %s" % (o[0] if o else "-", n[0] if n else "-", name[:100], verdict))
    total = len(set(old) | set(new))
    print("%d of %d kernels identical (%s build)" % (same, total, "diagnostics" if a.diag else "product"))
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
