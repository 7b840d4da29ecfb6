"""Print the compiled resource contract of every kernel of the product library (or of --lib FILE): VGPRs, AGPRs, SGPRs, spills, scratch, LDS,
workgroup size. A thin tool over tests/code_object.py; it needs hipcc and the LLVM tools, no GPU. Run it before and after a kernel edit:

    python tools/code_object_report.py --json before.json         # save the table
    ... edit, then ...
    python tools/code_object_report.py --diff before.json         # print every kernel and field that changed; exit status 1 if any did
    python tools/code_object_report.py --dirty                    # only kernels with scratch or VGPR spills
    python tools/code_object_report.py --match gemm256            # only kernels whose name contains the text
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import code_object  # noqa: E402

COLS = (("vgpr_count", "vgpr"), ("agpr_count", "agpr"), ("sgpr_count", "sgpr"), ("vgpr_spill_count", "vspill"), ("sgpr_spill_count", "sspill"),
        ("private_segment_fixed_size", "scratch"), ("group_segment_fixed_size", "lds"), ("max_flat_workgroup_size", "wg"), ("kernarg_segment_size", "karg"))


def table(recs):
    lines = [" ".join(f"{short:>7s}" for _, short in COLS) + "  kernel"]
    for name in sorted(recs):
        r = recs[name]
        lines.append(" ".join(f"{r[f]:7d}" for f, _ in COLS) + "  " + name + ("  [dynamic stack]" if r["uses_dynamic_stack"] else "")
                     + (f"  [wave{r['wavefront_size']}]" if r["wavefront_size"] != 64 else ""))
    return "\n".join(lines)


def diff(old, new):
    lines = []
    for name in sorted(set(old) | set(new)):
        if name not in new:
            lines.append(f"GONE     {name}")
        elif name not in old:
            lines.append(f"NEW      {name}")
        else:
            ch = [f"{f} {old[name].get(f)} -> {new[name][f]}" for f in code_object.FIELDS if old[name].get(f) != new[name][f]]
            if ch:
                lines.append(f"CHANGED  {name}: " + ", ".join(ch))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="library or code object to read (default: the product library, built if stale)")
    ap.add_argument("--json", metavar="FILE", help="write the table to FILE")
    ap.add_argument("--diff", metavar="FILE", help="print what changed against a table saved with --json")
    ap.add_argument("--dirty", action="store_true", help="print only kernels that use scratch or spill VGPRs")
    ap.add_argument("--match", metavar="TEXT", help="print only kernels whose name contains TEXT")
    a = ap.parse_args(argv)
    recs = code_object.kernels(a.lib)
    shown = {n: r for n, r in recs.items() if (not a.match or a.match in n) and (not a.dirty or r["private_segment_fixed_size"] or r["vgpr_spill_count"])}
    print(f"# {code_object.compiler_version()}")
    print(f"# {len(recs)} kernels, {sum(1 for r in recs.values() if r['private_segment_fixed_size'] or r['vgpr_spill_count'])} with scratch or VGPR spills")
    print(table(shown))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"compiler": code_object.compiler_version(), "kernels": recs}, f, indent=1, sort_keys=True)
            f.write("\n")
    if a.diff:
        with open(a.diff) as f:
            saved = json.load(f)
        lines = diff(saved["kernels"], recs)
        print(f"# against {a.diff} ({saved.get('compiler', '?')}): " + (f"{len(lines)} kernels differ" if lines else "no change"))
        print("\n".join(lines))
        return 1 if lines else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
