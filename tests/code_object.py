"""Reader of the compiled resource contract of every kernel in a HIP library: registers, spills, scratch, LDS, workgroup size.

    kernels()        -> {name: record} of the product library (built, unforced, when it is missing or stale)
    kernels(path)    -> the same for any shared library, object or bare gfx950 code object
    compile_device() -> compile a source string device-only for gfx950 (the reader's self-test uses it)

Metadata only: the records come from the `amdhsa.kernels` YAML document that the compiler writes into the NT_AMDGPU_METADATA note of every code
object. Nothing here reads an instruction stream. Names are demangled and normalised as tools/kernel_asm_diff.py does ("(anonymous namespace)::",
the leading "void " and the argument list dropped), so `gemm256_kernel<4, false, 128, false>` is a key.
A missing tool is an error, never a skip: llvm-objdump and llvm-readelf are looked up next to build.HIPCC (<rocm>/llvm/bin), c++filt on PATH.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unigen_amd import build  # noqa: E402

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
          "max_flat_workgroup_size", "wavefront_size", "uses_dynamic_stack", "kernarg_segment_size")
GFX_BUNDLE = "amdgcn-amd-amdhsa--gfx950"
ELF_MAGIC = b"\x7fELF"
EM_AMDGPU = 224


def llvm_tool(name: str) -> str:
    """<rocm>/llvm/bin/<name>, with <rocm> taken from build.HIPCC (<rocm>/bin/hipcc, symlinks resolved)"""
    hipcc = shutil.which(build.HIPCC) or build.HIPCC
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", name), os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", name)):
        if os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    raise FileNotFoundError(f"{name} not found under {rocm}/llvm/bin (derived from build.HIPCC = {build.HIPCC})")


def _cxxfilt() -> str:
    p = shutil.which("c++filt")
    if p is None:
        raise FileNotFoundError("c++filt not found on PATH")
    return p


def normalise(name: str) -> str:
    """the demangled name without the anonymous namespace, the return type and the argument list (as tools/kernel_asm_diff.py)"""
    name = name.replace("(anonymous namespace)::", "")
    return re.sub(r"^void ", "", name[:name.rindex("(")] if "(" in name else name)


def demangle(symbols: list[str]) -> list[str]:
    if not symbols:
        return []
    out = subprocess.run([_cxxfilt(), *symbols], capture_output=True, text=True, check=True).stdout.split("\n")
    return [normalise(n) for n in out[:len(symbols)]]


def compiler_version() -> str:
    """the two identifying lines of `hipcc --version` (HIP version, clang version)"""
    out = subprocess.run([build.HIPCC, "--version"], capture_output=True, text=True, check=True).stdout.split("\n")
    return "; ".join(ln.strip() for ln in out if ln.startswith("HIP version") or "clang version" in ln)


def _is_device_elf(path: str) -> bool:
    with open(path, "rb") as f:
        head = f.read(20)
    return head[:4] == ELF_MAGIC and int.from_bytes(head[18:20], "little") == EM_AMDGPU


def _metadata(code_object: str) -> list[dict]:
    """the amdhsa.kernels list of one gfx950 code object"""
    import yaml
    text = subprocess.run([llvm_tool("llvm-readelf"), "--notes", code_object], capture_output=True, text=True, check=True).stdout
    docs = re.findall(r"^\s*---\s*\n(.*?)^\s*\.\.\.\s*$", text, re.M | re.S)
    if not docs:
        raise RuntimeError(f"no AMDGPU metadata note in {code_object}")
    kernels = []
    for d in docs:
        kernels += (yaml.safe_load(d) or {}).get("amdhsa.kernels") or []
    return kernels


def kernels(lib: str | None = None) -> dict[str, dict]:
    """{normalised kernel name: {field: value for FIELDS, 'symbol': mangled name}} of every gfx950 kernel in `lib` (default: the product library).

    `lib` may be a host shared library or object with embedded offload bundles, or a bare device code object (hipcc --cuda-device-only --no-gpu-bundle-output -c)."""
    if lib is None:
        lib = build.build()
    lib = os.path.abspath(lib)
    if not os.path.isfile(lib):
        raise FileNotFoundError(lib)
    with tempfile.TemporaryDirectory(prefix="ug_code_object_") as tmp:
        if _is_device_elf(lib):
            objects = [lib]
        else:
            # llvm-objdump --offloading writes the bundles next to its input: run it on a copy, outside the tree
            copy = os.path.join(tmp, os.path.basename(lib))
            shutil.copyfile(lib, copy)
            subprocess.run([llvm_tool("llvm-objdump"), "--offloading", copy], cwd=tmp, capture_output=True, text=True, check=True)
            objects = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(GFX_BUNDLE))
            if not objects:
                raise RuntimeError(f"{lib} holds no {GFX_BUNDLE} offload bundle")
        raw = [k for o in objects for k in _metadata(o)]
    names = demangle([k[".name"] for k in raw])
    out = {}
    for name, k in zip(names, raw):
        if name in out:
            raise RuntimeError(f"kernel {name} appears twice in {lib}")
        missing = [f for f in FIELDS if f not in ("agpr_count", "uses_dynamic_stack") and "." + f not in k]
        if missing:
            raise RuntimeError(f"kernel {name}: metadata lacks {missing}")
        rec = {f: k.get("." + f, 0) for f in FIELDS}
        rec["uses_dynamic_stack"] = bool(rec["uses_dynamic_stack"])
        rec["symbol"] = k[".name"]
        out[name] = rec
    return out


def compile_device(source: str, out_dir: str, stem: str = "k", flags: tuple = ()) -> str:
    """compile `source` device-only for gfx950 into out_dir/<stem>.co with the product's flags; returns the code object's path"""
    src = os.path.join(out_dir, stem + ".hip")
    obj = os.path.join(out_dir, stem + ".co")
    with open(src, "w") as f:
        f.write(source)
    r = subprocess.run([build.HIPCC, *build.FLAGS, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj], capture_output=True, text=True, cwd=out_dir)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
    return obj
