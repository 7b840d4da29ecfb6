"""ctypes binding of libunigen_hip.so, derived at import from the C ABI's one declaration: include/unigen_hip.h.

Constants, descriptor structs and prototypes are parsed from the header text (a closed C subset; anything else raises at import),
so a symbol is declared in one place. The product path has no fallback: if the shared library is missing or does not load,
importing the ops raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

from . import build as _build

HEADER = _build.HEADER
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UG_LIB_PATH") or os.path.join(_HERE, "libunigen_hip.so")      # UG_LIB_PATH: an alternative build (A/B tools only)


class UniGenHipError(RuntimeError):
    pass


# the closed type map of the header; `void` and `char` occur only behind pointers, ug_stream_t joins through its typedef
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
            "int16_t": C.c_int16, "float": C.c_float, "double": C.c_double}
_TYPE_THEN_NAMES, _NAME = re.compile(r"(?:const\s+)?(\w+)\b\s*(.+)"), re.compile(r"\s*(\*?)\s*(?:const\s+)?(\w+)\s*")      # `const T` + `* a` or `a, b, c`


def _bad(what: str, decl: str):
    raise UniGenHipError(f"unigen_hip.h: {what}: `{decl}`")


def _declarators(decl: str, types: dict, where: str) -> list:
    """`const T* a` or `T a, b, c` -> [(name, ctype)]. Every pointer is a c_void_p: that argtype takes integer device addresses, None,
    byref(struct), ctypes arrays and typed pointers."""
    m = _TYPE_THEN_NAMES.fullmatch(decl)
    names = [_NAME.fullmatch(d) for d in m.group(2).split(",")] if m else [None]
    if not all(names):
        _bad(f"cannot split `{decl}`", where)
    base = m.group(1)
    if base not in types and not (base in ("void", "char") and all(n.group(1) for n in names)):
        _bad(f"unknown type `{base}`", where)
    return [(n.group(2), C.c_void_p if n.group(1) else types[base]) for n in names]


def parse_header(text: str):
    """C header text -> (constants {name: int}, structs {C name: ctypes.Structure}, signatures {name: (restype, [argtypes])}, twins {twin: base}).
    Understands `#define UG_X <int>`, anonymous enums, `typedef void* T;`, `typedef struct ug_x {...} ug_x;` and prototypes of `ug_*`; raises
    UniGenHipError, quoting the declaration, on anything else."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, structs, sigs, types = {}, {}, {}, dict(_SCALARS)
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = re.fullmatch(r"#\s*define\s+(UG_\w+)\s+(\S.*?)", line.strip())
        if m:
            if not re.fullmatch(r"-?(0x[0-9a-fA-F]+|\d+)", m.group(2)):
                _bad("not an integer constant", line.strip())
            consts[m.group(1)] = int(m.group(2), 0)
    text, in_extern_c = re.subn(r'extern\s+"C"\s*\{', " ", re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M))
    if in_extern_c:
        text, closed = re.subn(r"\}\s*\Z", " ", text)
        if not closed:
            _bad('`extern "C" {` is not closed at the end', " ".join(text.split())[-80:])
    decls, pos = [], 0
    for m in re.finditer(r"\s*((?:[^;{}]|\{[^{}]*\})*);", text):      # a `;` inside a struct's braces (one level) does not end the declaration
        if m.start() != pos:
            break
        decls.append(" ".join(m.group(1).split()))
        pos = m.end()
    if text[pos:].strip():
        _bad("text after the last declaration", " ".join(text[pos:].split())[:200])
    for decl in decls:
        if m := re.fullmatch(r"enum \{(.*)\}", decl):
            value = -1
            for item in filter(None, (i.strip() for i in m.group(1).split(","))):
                im = re.fullmatch(r"(\w+)(?:\s*=\s*(-?\d+))?", item) or _bad("cannot read the enumerator", item)
                consts[im.group(1)] = value = int(im.group(2)) if im.group(2) else value + 1
        elif m := re.fullmatch(r"typedef void ?\* ?(\w+)", decl):
            types[m.group(1)] = C.c_void_p
        elif m := re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", decl):
            if m.group(1) != m.group(3):
                _bad("struct tag and typedef name differ", decl)
            fields = [f for d in m.group(2).split(";") if d.strip() for f in _declarators(d.strip(), types, decl)]
            types[m.group(1)] = structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields, "__doc__": f"struct {m.group(1)} of include/unigen_hip.h"})
        elif m := re.fullmatch(r"(?:const )?(\w+) ?(\*?) ?(ug_\w+) ?\(([^()]*)\)", decl):
            ret, ptr, name, params = m.groups()
            if (ret != "char") if ptr else (ret not in _SCALARS):
                _bad(f"unknown return type `{ret}{ptr}`", decl)
            args = [] if params.strip() == "void" else [_declarators(p.strip(), types, decl) for p in params.split(",")]
            if name in sigs or any(len(a) != 1 for a in args):
                _bad("declared twice" if name in sigs else "cannot split the parameters", decl)
            sigs[name] = (C.c_char_p if ptr else _SCALARS[ret], [a[0][1] for a in args])
        else:
            _bad("not a declaration this binding understands", decl)
    stray = set(re.findall(r"\b(ug_\w+)\s*\(", text)) - set(sigs)
    if stray:
        _bad("`ug_*(` outside a prototype", ", ".join(sorted(stray)))
    # fp32 verification twins: `S_f32` mirrors `S` or `S_bf16` when that is declared too, and must have its signature
    twins = {n: b for n in sigs if n.endswith("_f32") for b in (n[:-4] + "_bf16", n[:-4]) if b in sigs}
    for twin, base in twins.items():
        if sigs[twin] != sigs[base]:
            _bad(f"the fp32 twin's prototype differs from that of {base}", twin)
    return consts, structs, sigs, twins


def _read_header() -> str:
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise UniGenHipError(f"{HEADER}: the C ABI's header is missing, and the binding is derived from it ({e})") from e


_CONSTANTS, STRUCTS, SIGNATURES, _F32_TWINS = parse_header(_read_header())
globals().update(_CONSTANTS)                                                                          # UG_OK, UG_ERR_*, UG_EPI_*, UG_DT_*, UG_FLOW_*, UG_OPTIM_CHUNK, ...
globals().update({k[3:]: v for k, v in _CONSTANTS.items() if k.startswith("UG_EPI_")})                 # EPI_BIAS, ...: the short names the callers use
F32_TWIN_OF = {base: twin for twin, base in _F32_TWINS.items()}
GemmDesc, ConvDesc, VaeTile, VaeBlendDesc = (STRUCTS[n] for n in ("ug_gemm_desc", "ug_conv_desc", "ug_vae_tile", "ug_vae_blend_desc"))
OptimTensor, AdamwGroup, OptimTensorLP, AdamwGroupLP = (STRUCTS[n] for n in ("ug_optim_tensor", "ug_adamw_group", "ug_optim_tensor_lp", "ug_adamw_group_lp"))


def optim_tensor(*, grad: int, grad_dtype: int, numel: int, param: int = 0, param_dtype: int = UG_DT_F32, master: int = 0, exp_avg: int = 0,
                 exp_avg_sq: int = 0, group: int = 0) -> OptimTensor:
    """One ug_optim_tensor from raw device addresses (0 = NULL): any element alignment, any of the four (grad dtype, master) forms."""
    return OptimTensor(param or None, grad or None, master or None, exp_avg or None, exp_avg_sq or None, numel, param_dtype, grad_dtype, group, 0)


def bind(cdll: C.CDLL) -> C.CDLL:
    """Give every entry point of a build of the library its restype / argtypes."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(cdll, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    return cdll


_lib = None


def load() -> C.CDLL:
    """Load the HIP library (once). Raises if it has not been built: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        # a clean clone carries no binaries: build the product library once, in-tree (about 30 s); there is no CPU fallback for the hot path
        if os.environ.get("UG_LIB_PATH"):
            raise UniGenHipError(f"UG_LIB_PATH={LIB_PATH} not found (probe library: `python -m unigen_amd.build --probe`)")
        try:
            _build.build()          # serialised across processes by a file lock; outputs appear atomically (os.replace)
        except Exception as e:      # no hipcc, compile error: fail loudly, never fall back
            raise UniGenHipError(f"{LIB_PATH} not found and `python -m unigen_amd.build` (hipcc --offload-arch=gfx950) failed: {e}. "
                                 "unigen_amd has no CPU fallback for the hot path.") from e
    # The library links libamdhip64 by SONAME. PyTorch-ROCm ships its own copy of the HIP runtime: it has to be in the process first so
    # that both resolve to ONE runtime (loaded the other way round, the system runtime and torch's each keep their own device state and
    # launches fail with "no ROCm-capable device is detected").
    import torch  # noqa: F401
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def check(rc: int, what: str) -> None:
    if rc != UG_OK:
        msg = load().ug_last_error()
        raise UniGenHipError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def call(name: str, *args) -> None:
    """Call the entry point `name` of the loaded library; a status other than UG_OK raises with the library's message."""
    rc = getattr(load(), name)(*args)
    if rc:
        check(rc, name)
