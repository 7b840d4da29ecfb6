"""CPU tests of the header parser behind unigen_amd/lib.py (`parse_header`), on header snippets given as strings: what it derives from the closed
C subset of include/unigen_hip.h, and that everything outside that subset raises, quoting the declaration, instead of being skipped."""
import ctypes as C

import pytest

from unigen_amd import lib

I32, I64, VP = C.c_int32, C.c_int64, C.c_void_p
PRELUDE = "#include <stdint.h>\ntypedef void* ug_stream_t; /* hipStream_t */\n"


def test_prototypes_wrapped_lines_void_and_the_closed_type_map():
    consts, structs, sigs, twins = lib.parse_header(PRELUDE + """
        /* wrapped over three lines, every scalar of the type map */
        int ug_wrapped(const void* x, int64_t ldx, int32_t n,
                       uint32_t a, uint64_t b, float c, double d,
                       const uint8_t* img, int16_t* dx, const float* t, ug_stream_t stream);
        int64_t ug_bytes(void);
        const char* ug_text(void);
        int ug_version(void);""")
    assert sigs == {"ug_wrapped": (I32, [VP, I64, I32, C.c_uint32, C.c_uint64, C.c_float, C.c_double, VP, VP, VP, VP]), "ug_bytes": (I64, []),
                    "ug_text": (C.c_char_p, []), "ug_version": (I32, [])}
    assert consts == {} and structs == {} and twins == {}


def test_constants_from_enums_and_defines():
    consts, _, sigs, _ = lib.parse_header("""
        #ifndef GUARD_H
        #define GUARD_H
        #ifdef __cplusplus
        extern "C" {
        #endif
        enum { UG_OK = 0, UG_ERR_BAD_SHAPE = -1,
               UG_ERR_HIP = -4 };
        enum { UG_A, UG_B, UG_C = 7, UG_D };      /* implicit values count on from the previous enumerator */
        #define UG_CHUNK 65536
        #define UG_MASK 0x1f
        int ug_version(void);
        #ifdef __cplusplus
        }
        #endif
        #endif""")
    assert consts == dict(UG_OK=0, UG_ERR_BAD_SHAPE=-1, UG_ERR_HIP=-4, UG_A=0, UG_B=1, UG_C=7, UG_D=8, UG_CHUNK=65536, UG_MASK=31) and list(sigs) == ["ug_version"]
    with pytest.raises(lib.UniGenHipError, match=r"not an integer constant.*UG_SCALE 0\.5f"):
        lib.parse_header("#define UG_SCALE 0.5f\n")


def test_structs_comma_declarators_and_nesting_by_value():
    _, structs, sigs, _ = lib.parse_header(PRELUDE + """
        typedef struct ug_tile {
            const void* p;          /* a pointer member */
            int64_t H, W;
            int32_t a, b, c; float* q;
        } ug_tile;
        typedef struct ug_pair { ug_tile T, U; void* out; int64_t M, N, K; uint32_t step; uint64_t seed; } ug_pair;
        int ug_blend(const ug_pair* d, ug_stream_t stream);""")
    T, P = structs["ug_tile"], structs["ug_pair"]
    assert T._fields_ == [("p", VP), ("H", I64), ("W", I64), ("a", I32), ("b", I32), ("c", I32), ("q", VP)] and issubclass(T, C.Structure)
    assert P._fields_ == [("T", T), ("U", T), ("out", VP), ("M", I64), ("N", I64), ("K", I64), ("step", C.c_uint32), ("seed", C.c_uint64)]
    assert C.sizeof(T) == 48 and P.U.offset == 48 and P.out.offset == 96 and P.seed.offset == 136 and C.sizeof(P) == 144
    assert sigs == {"ug_blend": (I32, [VP, VP])}
    d = P()
    d.U.H, d.K = 5, 7
    assert (d.U.H, d.T.H, d.K) == (5, 0, 7)


def test_a_call_inside_a_comment_declares_nothing():
    _, _, sigs, _ = lib.parse_header("/* see ug_fake(x, y); and\n ug_other( */\nint ug_real(int32_t n);   // like ug_fake2(n)\n")
    assert list(sigs) == ["ug_real"]


@pytest.mark.parametrize("snippet, quoted", [
    ("int ug_f(const void* x, size_t n);", r"unknown type `size_t`.*`int ug_f\(const void\* x, size_t n\)`"),                    # not in the type map
    ("typedef struct ug_s { int64_t n; ug_missing t; } ug_s;", r"unknown type `ug_missing`.*typedef struct ug_s"),            # a struct used before it exists
    ("int ug_f(void x);", r"unknown type `void`.*ug_f"),                                                                     # void only behind a pointer
    ("void ug_f(int32_t n);", r"unknown return type `void`.*`void ug_f\(int32_t n\)`"),
    ("int ug_f(unsigned int n);", r"cannot split `unsigned int n`.*ug_f"),
    ("int ug_f(int32_t (*cb)(int32_t));", r"not a declaration.*ug_f"),                                                       # a function pointer
    ("int ug_f(int32_t n); int ug_f(int32_t n);", r"declared twice"),
    ("int helper(int32_t n);", r"not a declaration this binding understands.*`int helper\(int32_t n\)`"),                      # not a ug_ symbol
    ("typedef struct ug_s { int32_t n; } ug_t;", r"tag and typedef name differ"),
    ("static inline int ug_f(int32_t n) { return n; }", r"ug_f"),                                                            # a definition is not a declaration
    ("int ug_f(int32_t n)", r"after the last declaration.*ug_f"),                                                            # the `;` is missing
    ("union ug_u { int32_t a; float b; };", r"not a declaration"),
])
def test_what_the_parser_does_not_recognise_raises_and_quotes_it(snippet, quoted):
    with pytest.raises(lib.UniGenHipError, match=quoted):
        lib.parse_header(PRELUDE + "int ug_version(void);\n" + snippet + "\n")


def test_fp32_twins_are_derived_and_must_repeat_the_base_prototype():
    ok = PRELUDE + """
        int ug_relu(const void* x, void* y, int64_t n, ug_stream_t stream);
        int ug_relu_f32(const void* x, void* y, int64_t n, ug_stream_t stream);
        int ug_gemm_bf16(const void* d, ug_stream_t stream);
        int ug_gemm_f32(const void* d, ug_stream_t stream);
        int ug_add_rowbcast_f32(void* x, const float* table, int64_t rows, ug_stream_t stream);
        int ug_add_rowbcast_f32_f32(void* x, const float* table, int64_t rows, ug_stream_t stream);
        int ug_bicubic_f32(const float* x, float* out, ug_stream_t stream);"""
    twins = lib.parse_header(ok)[3]
    assert twins == {"ug_relu_f32": "ug_relu", "ug_gemm_f32": "ug_gemm_bf16", "ug_add_rowbcast_f32_f32": "ug_add_rowbcast_f32"}      # ug_add_rowbcast_f32, ug_bicubic_f32: bases
    for bad in ("int ug_relu_f32(const void* x, void* y, int32_t n, ug_stream_t stream);",      # i32 where the base takes i64
                "int ug_relu_f32(const void* x, void* y, int64_t n, float s, ug_stream_t stream);",
                "int64_t ug_relu_f32(const void* x, void* y, int64_t n, ug_stream_t stream);"):
        with pytest.raises(lib.UniGenHipError, match=r"twin's prototype differs from that of ug_relu.*ug_relu_f32"):
            lib.parse_header(ok.replace("int ug_relu_f32(const void* x, void* y, int64_t n, ug_stream_t stream);", bad))


def test_the_shipped_header_binds_and_a_missing_one_is_named(monkeypatch, tmp_path):
    assert len(lib.SIGNATURES) >= 154 and len(lib.STRUCTS) >= 8 and lib.F32_TWIN_OF["ug_gemm_bf16"] == "ug_gemm_f32"
    assert all(lib.SIGNATURES[t] == lib.SIGNATURES[b] for t, b in lib._F32_TWINS.items())
    assert "ug_add_rowbcast_f32" not in lib._F32_TWINS and "ug_bicubic_f32" not in lib._F32_TWINS
    assert (lib.UG_OK, lib.UG_ERR_HIP, lib.EPI_QKV_ROPE, lib.UG_EPI_QKV_ROPE, lib.UG_OPTIM_CHUNK, lib.UG_FLOW_MODE) == (0, -4, 5, 5, 65536, 4)
    # the header's own rule: every pointer is a device pointer unless the name ends in _host - the three host parameters say so
    hdr = open(lib.HEADER).read()
    assert "int32_t* sweeps_host" in hdr and "const float* mean_host, const float* std_host" in hdr
    monkeypatch.setattr(lib, "HEADER", str(tmp_path / "nowhere" / "unigen_hip.h"))
    with pytest.raises(lib.UniGenHipError, match="nowhere/unigen_hip.h"):
        lib._read_header()


def test_bind_types_any_build_of_the_library_and_call_names_the_symbol_it_called():
    from unigen_amd import ops
    import torch
    lib.load()                                                             # builds the library on a clean checkout
    cdll = lib.bind(C.CDLL(lib.LIB_PATH))                                  # a second handle, bound the way the A/B tools bind other builds
    assert cdll.ug_relu.argtypes == [VP, VP, I64, VP] and cdll.ug_gemm_workspace_bytes.restype is I64 and cdll.ug_last_error.restype is C.c_char_p
    assert cdll.ug_relu(None, None, 8, None) == lib.UG_ERR_BAD_SHAPE
    with pytest.raises(lib.UniGenHipError, match=r"^ug_relu failed \(code -1\)"):
        ops._call("ug_relu", torch.bfloat16, None, None, 8, None)
    with pytest.raises(lib.UniGenHipError, match=r"^ug_relu_f32 failed \(code -1\)"):          # the fp32 path reports the twin it called
        ops._call("ug_relu", torch.float32, None, None, 8, None)
    with pytest.raises(lib.UniGenHipError, match=r"^ug_gemm_f32 failed"):
        ops._call("ug_gemm_bf16", torch.float32, None, None)
    assert ops._fn("ug_add_bf16", torch.float32) is lib.load().ug_add_f32 and ops._fn("ug_add_bf16", torch.bfloat16) is lib.load().ug_add_bf16
