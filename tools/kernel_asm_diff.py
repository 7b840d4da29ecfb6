"""Per-kernel comparison of two device-only assembly listings (hipcc --cuda-device-only -S): the proof that a source refactor left the machine code alone.
For every kernel present on both sides: the instruction stream (symbol names and function-local label numbers normalised) and the kernel descriptor
(.amdhsa_* directives: VGPR / AGPR / SGPR counts, scratch, LDS; plus the compiler's Occupancy / ScratchSize / spill comments) must be equal.
    usage: python tools/kernel_asm_diff.py A.s B.s [B2.s ...] [--pair 'NAME_IN_A=NAME_IN_B' ...] [--rename OLD=NEW ...]
--rename rewrites kernel names of the B side before matching (a kernel that moved to another name); --pair matches two differently spelled
instantiations (names as printed, without the anonymous namespace and the argument list). Exit status 1 if any matched kernel differs."""
import re, subprocess, sys

CXXFILT = "c++filt"


def kernels(path):
    """{demangled name: (instructions, descriptor lines)} of one listing"""
    text = open(path).read()
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    names = subprocess.run([CXXFILT, *syms], capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for sym, name in zip(syms, names):
        name = name.replace("(anonymous namespace)::", "")
        name = re.sub(r"^void ", "", name[:name.rindex("(")] if "(" in name else name)
        body = text[text.index("\n" + sym + ":") + len(sym) + 2:]
        body = body[:body.index(".Lfunc_end")]
        ins = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip().replace(sym, "KERNEL")
            if ln:
                ins.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        desc = text[text.index(".amdhsa_kernel " + sym):]
        desc = [ln.strip().replace(sym, "KERNEL") for ln in desc[:desc.index(".end_amdhsa_kernel")].split("\n")]
        stats = text[text.index("\n" + sym + ":"):]
        stats = stats[stats.index(".Lfunc_end"):]
        stats = re.findall(r"^; ((?:NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|SGPRBlocks|VGPRBlocks|codeLenInByte)\b.*)$",
                           stats[:stats.index(".amdhsa_kernel")] if ".amdhsa_kernel" in stats else stats, re.M)
        out[name] = (ins, desc + stats)
    return out


def main(argv):
    files = [a for a in argv if not a.startswith("--") and "=" not in a]
    opt = lambda flag: [argv[i + 1].split("=", 1) for i, a in enumerate(argv[:-1]) if a == flag]
    A = kernels(files[0])
    B = {}
    for f in files[1:]:
        for name, kd in kernels(f).items():
            for old, new in opt("--rename"):
                name = name.replace(old, new)
            B[name] = kd
    pairs = dict(opt("--pair"))
    bad = 0
    for na in sorted(A):
        nb = pairs.get(na, na)
        if nb not in B:
            print(f"ONLY IN A            {na}")
            continue
        (ia, da), (ib, db) = A[na], B.pop(nb)
        code = "identical" if ia == ib else f"DIFFERS ({len(ia)} vs {len(ib)} lines)"
        desc = "identical" if da == db else "DIFFERS: " + "; ".join(f"{x} | {y}" for x, y in zip(da, db) if x != y)
        bad += ia != ib or da != db
        print(f"code {code:10s} descriptor {desc:10s} {len(ia):6d} lines   {na}" + (f"  ==  {nb}" if nb != na else ""))
    for nb in sorted(B):
        print(f"ONLY IN B            {nb}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
