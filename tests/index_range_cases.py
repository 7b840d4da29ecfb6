"""Case tables and helpers of the index-range sweep (tests/test_index_range_gpu.py runs them on the device, tests/test_index_range_cases_cpu.py
checks on the host that every entry is what it claims to be): kernels at the top of their index ranges - row strides at the largest admitted
value, batch strides that put a sample past byte offset 2^32, packed convolution coordinates with their high bits set.

FAR VIEWS. One arena per test module (torch.empty: nothing is initialised), operands carved out of it with as_strided at huge row / batch
strides, the first operand at least 2^31 bytes into the arena so that an offset wrongly cut or sign-extended to 32 bits still lands inside the
allocation: a bug shows as wrong values, never as a fault. Only the elements the kernel is entitled to read are written, and SENT_COLS sentinel
elements behind every output row. A far launch must give the bits of the same values launched at compact strides, and that compact launch is
first judged against float64 by the sweeps' own judging functions.

A layout here is a dict name -> element offset of the operand's [batch 0, row 0, column 0] inside the arena; every operand of a case shares the
case's row stride `rs` and batch stride `bs` (elements)."""
import functools

import torch

from tests import vae_kernel_ref as VR

GIB = 1 << 30
MEMORY_CAP = 16 * GIB                    # no test may hold more device memory than this
SENT_COLS = 64                           # sentinel elements behind every output row
ARENA_BASE = (1 << 30) + 4096            # elements: the first operand of a bf16 case starts 2^31 + 8192 bytes into the arena

# ----------------------------------------------------------------------------------------------------------------------------------
# ug_flash_attn_fwd / _fwd_lse / _bwd: the row-stride rule and the cases at its edge
# ----------------------------------------------------------------------------------------------------------------------------------
ATTN_RS_LIMIT = 1 << 24                  # include/unigen_hip.h: 0 < row stride < 2^24 elements
ATTN_RS_SOUND = ((1 << 31) - 120) // 63  # what the kernels' 32-bit tile offsets hold: 63 rs + 120 < 2^31
ATTN_RS_FAR = ATTN_RS_LIMIT - 16         # the largest admitted stride that is a multiple of 16 (the buffer-form DMAs need that)
ATTN_BS_FAR = 136 * ATTN_RS_FAR          # whole rows; 2 bytes x this is past 2^32: batch 1 of every operand lies beyond byte offset 2^32
ATTN_FWD_ROW_STRIDES = ("q_rs", "k_rs", "v_rs", "o_rs")
ATTN_BWD_ROW_STRIDES = ("q_rs", "k_rs", "v_rs", "o_rs", "do_rs", "dq_rs", "dk_rs", "dv_rs")
ATTN_OPERANDS = ("k", "v", "q", "do", "o", "dq", "dk", "dv")
ATTN_OUTPUTS = ("o", "dq", "dk", "dv")


def bufd_ok(k_rs: int, v_rs: int, Lkv: int) -> bool:
    """flash_attn_fwd_impl's condition for the buffer-form K / V DMAs at head width 64, restated"""
    return k_rs == v_rs and k_rs % 16 == 0 and Lkv * k_rs * 2 < (1 << 31)


def _attn(name, dh, Lq, Lkv, rs=None, bs=None, B=2, H=2):
    D = H * dh
    compact_rs = 8 * D + 4 * SENT_COLS                      # K | V | Q | dO | O .. | dQ .. | dK .. | dV .. in one row
    rs = compact_rs if rs is None else rs
    return dict(name=name, dh=dh, B=B, H=H, Lq=Lq, Lkv=Lkv, rs=rs, bs=(max(Lq, Lkv) + 6) * rs if bs is None else bs, seed=6100 + dh + 7 * Lq + Lkv)


# part 1: every operand at the largest admitted row stride, batch 1 past 2^32 bytes. dh 64: Lkv = 64 is the last length at which the dispatcher
# takes the buffer-form DMAs at this stride (64 rs 2 < 2^31), Lkv = 65 the first that takes the pointer form, with one ragged tile.
ATTN_FAR_CASES = [
    _attn("dh128-64x64", 128, 64, 64, ATTN_RS_FAR, ATTN_BS_FAR),
    _attn("dh128-130x65", 128, 130, 65, ATTN_RS_FAR, ATTN_BS_FAR),
    _attn("dh128-130x130", 128, 130, 130, ATTN_RS_FAR, ATTN_BS_FAR),
    _attn("dh64-64x64-buf", 64, 64, 64, ATTN_RS_FAR, ATTN_BS_FAR),
    _attn("dh64-130x64-buf", 64, 130, 64, ATTN_RS_FAR, ATTN_BS_FAR),
    _attn("dh64-64x65-ptr", 64, 64, 65, ATTN_RS_FAR, ATTN_BS_FAR),
    _attn("dh64-130x130-ptr", 64, 130, 130, ATTN_RS_FAR, ATTN_BS_FAR),
]
# part 3: the cfg3 B = 8 situation shrunk - compact rows, a batch stride of more than 2^31 elements, so the LAST batch of every operand starts
# past byte offset 2^32 while batch 0 lies below it
ATTN_BATCH_CASES = [
    _attn("dh128-300x300-batch", 128, 300, 300, bs=(1 << 31) + 8 * (8 * 256 + 4 * SENT_COLS)),
    _attn("dh64-200x300-batch", 64, 200, 300, bs=(1 << 31) + 8 * (8 * 128 + 4 * SENT_COLS)),
]


def attn_layout(c: dict) -> dict:
    """element offsets of the eight operands of an attention case: K and V interleaved in the same rows, Q / dO / O / dQ / dK / dV behind them in
    the same rows, SENT_COLS sentinel elements behind every output's D columns"""
    D = c["H"] * c["dh"]
    cols = dict(k=0, v=D, q=2 * D, do=3 * D, o=4 * D, dq=5 * D + SENT_COLS, dk=6 * D + 2 * SENT_COLS, dv=7 * D + 3 * SENT_COLS)
    assert cols["dv"] + D + SENT_COLS <= c["rs"] and all(v % 8 == 0 for v in cols.values())
    return {n: ARENA_BASE + v for n, v in cols.items()}


def attn_rows(c: dict, name: str) -> int:
    return c["Lkv"] if name in ("k", "v", "dk", "dv") else c["Lq"]


def view_extent(off: int, rs: int, bs: int, B: int, rows: int, width: int) -> int:
    """one past the last element of a [B, rows, width] view at element offset `off` with strides (bs, rs, 1)"""
    return off + (B - 1) * bs + (rows - 1) * rs + width


def attn_arena_elems(c: dict) -> int:
    D = c["H"] * c["dh"]
    return max(view_extent(off, c["rs"], c["bs"], c["B"], attn_rows(c, n), D + SENT_COLS) for n, off in attn_layout(c).items())


def assert_disjoint(spans) -> None:
    """[(first, one past last)] element intervals of one arena: none may overlap another"""
    spans = sorted(spans)
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], ("two operands overlap in the arena", a, b)


def far_view(arena: torch.Tensor, off: int, rs: int, bs: int, B: int, rows: int, width: int) -> torch.Tensor:
    assert view_extent(off, rs, bs, B, rows, width) <= arena.numel(), "the view would leave the arena"
    return arena.as_strided((B, rows, width), (bs, rs, 1), off)


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_flash_attn_fwd_wide (+ _f32): K / V at the largest admitted row stride, and the 4096^2 canvas' key count
# ----------------------------------------------------------------------------------------------------------------------------------
WIDE_RS_FAR = (1 << 24) - 8
WIDE_BS_FAR = 72 * WIDE_RS_FAR           # whole rows; batch 1 past byte offset 2^32 in bf16 and in fp32, two fp32 batches inside 12 GiB
WIDE_FAR_CASES = [dict(name=f"wide-70x{Lkv}", B=2, H=1, Lq=70, Lkv=Lkv, rs=WIDE_RS_FAR, bs=WIDE_BS_FAR, seed=6400 + Lkv) for Lkv in (32, 33, 70)]
WIDE_COLS = dict(k=0, v=512, q=1024, o=1536)                  # + SENT_COLS behind o
WIDE_CANVAS = dict(name="wide-130x262144", B=1, H=1, Lq=130, Lkv=262144, seed=6500)       # H W of the mid block of a 4096^2 decode


def wide_layout(c: dict, itemsize: int) -> dict:
    """element offsets (of `itemsize`-byte elements) of k, v, q, o: the first operand 2^31 bytes into the arena whatever the element size"""
    base = (1 << 31) // itemsize + 4096
    return {n: base + v for n, v in WIDE_COLS.items()}


def wide_arena_bytes(c: dict, itemsize: int) -> int:
    lay = wide_layout(c, itemsize)
    return itemsize * max(view_extent(lay[n], c["rs"], c["bs"], c["B"], c["Lkv"] if n in "kv" else c["Lq"], 512 + SENT_COLS) for n in lay)


# ----------------------------------------------------------------------------------------------------------------------------------
# the 256^2 convolution route: gemm256_kernel<CONV> keeps a staging row's output pixel as b << 24 | oy << 12 | ox (8 | 12 | 12 bits) and unpacks
# input coordinates that the host bounds by H, W < 2048; ug_conv2d_nhwc guards the route with B < 256, H, W < 2048, Ho, Wo < 4096.
# The cases with the high bits set are the last five rows of vae_kernel_ref.CONV256_CASES; these lie just OUTSIDE a limit: they must run on the
# 128^2 kernel (and on the fp32 twin), where they are judged like any other geometry.
# ----------------------------------------------------------------------------------------------------------------------------------
CONV256_HIGH_BITS = 5                    # how many rows at the end of VR.CONV256_CASES this sweep added
CONV256_OUTSIDE = [
    VR._c256(1, 8, 2048, 128, 3, 3, 1, 1, 1, 1, 16, 4096),        # W = 2048, Wo = 4096 through the folded upsampling
    VR._c256(256, 8, 8, 128, 3, 3, 1, 1, 1, 0, 8, 8),             # B = 256
]


def conv_pack(b, oy, ox, ox_bits=12, oy_bits=12):
    """the packed output pixel of a staging row, with fields of the given widths (12 | 12: the kernel's)"""
    return (b << 24) | ((oy & ((1 << oy_bits) - 1)) << 12) | (ox & ((1 << ox_bits) - 1))


def conv_unpack(p):
    return p >> 24, (p >> 12) & 0xFFF, p & 0xFFF


def conv_coordinate_slip(out: torch.Tensor, field: str, bits: int = 11) -> torch.Tensor:
    """out [B, Ho, Wo, C] as a kernel would produce it whose packed `field` ('ox', 'oy' or 'b') kept only `bits` bits (b: of its 8): every output
    pixel receives the value of the pixel its truncated coordinates name"""
    B, Ho, Wo, _ = out.shape
    b, oy, ox = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    if field == "b":
        b = b & ((1 << bits) - 1)
    else:
        pb, py, px = conv_unpack(conv_pack(b, oy, ox, ox_bits=bits if field == "ox" else 12, oy_bits=bits if field == "oy" else 12))
        b, oy, ox = pb, py, px
    return out[b, oy, ox]


# ----------------------------------------------------------------------------------------------------------------------------------
# ug_gemm_bf16: each operand past byte offset 2^32 from its own base - by group stride, or by leading dimension - at small shapes, on both
# tiles. A case is a compact case of tests/test_fuzz_gemm_gpu.py (`base`, whose buffers gemm_operands draws) and the same descriptor with
# some strides replaced (`far`); `crosses` names the operands whose last element then lies beyond 2^32 bytes from the operand's base.
# ----------------------------------------------------------------------------------------------------------------------------------
GEMM_LD_FAR = 4210760                    # elements: 512 rows of it span 2^32 bytes (the leading dimension of the sweep's "A tile spans 2^31 bytes")
GEMM_GS_FAR = (1 << 31) + 4096           # elements: group 1 starts past byte offset 2^32
GEMM_ARENA_BYTES = 7 * GIB
GEMM_OPERANDS = ("a", "w", "bias", "gate", "r", "c")
_GEMM_LD = dict(a="lda", w="ldw", gate="gate_ld", r="ldr", c="ldc")
_GEMM_GS = dict(a="a_gstride", w="w_gstride", bias="bias_gstride", gate="gate_gstride", r="r_gstride", c="c_gstride")


@functools.lru_cache(maxsize=None)
def gemm_far_cases():
    """built once per process (the compact cases come from tests/test_fuzz_gemm_gpu.py's `_case`); treat the result as read-only"""
    from tests import fwd_ref as FR
    from tests.test_fuzz_gemm_gpu import _case
    gs = {k: GEMM_GS_FAR for k in _GEMM_GS.values()}
    ld = GEMM_LD_FAR
    # ldc = N + SENT_COLS where the leading dimension stays compact: the sentinel columns behind a far C row are that row's own padding
    mk = lambda base, far, crosses, split=False: dict(name=base["name"], base=base, far=dict(base, **far), crosses=crosses, split=split)
    return [
        mk(_case("group strides, res_gate per row, R apart", (256, 1, 1, 0, 3), 300, 520, 192, FR.EPI_RES_GATE, groups=2, rps=1, ldc_extra=SENT_COLS), gs,
           ("a", "w", "bias", "gate", "r", "c")),
        mk(_case("group strides, res_scale, R = C", (256, 1, 1, 0, 3), 300, 520, 64, FR.EPI_RES_SCALE, groups=2, alias=True, ldc_extra=SENT_COLS),
           {k: v for k, v in gs.items() if k != "gate_gstride"}, ("a", "w", "bias", "c")),
        mk(_case("ldw -> the 128^2 kernel", (128, 1, 1, 0, 0), 300, 520, 192, FR.EPI_BIAS_GELU, ldc_extra=SENT_COLS), dict(ldw=ld), ("w",)),
        mk(_case("ldc, ldr, gate_ld; split-K", (256, 1, 8, 8, 3), 512, 520, 6144, FR.EPI_RES_GATE, rps=1),
           dict(ldc=ld, ldr=ld, gate_ld=ld), ("c", "r", "gate"), split=True),
        mk(_case("ldc, R = C", (256, 1, 1, 0, 3), 520, 520, 128, FR.EPI_RES_SCALE, alias=True), dict(ldc=ld, ldr=ld), ("c",)),
    ]


def gemm_operand_shape(c: dict, op: str):
    """(groups, rows, width) of the elements of operand `op` a kernel may touch (C, and an R it aliases: the written columns)"""
    rows = dict(a=c["a_rows"], w=c["N"], bias=1, gate=c["gate_rows"], r=c["c_rows"], c=c["c_rows"])[op]
    return max(c["groups"], 1), rows, c["K"] if op in ("a", "w") else c["N"]


def gemm_operand_strides(c: dict, op: str):
    """(group stride, leading dimension) of operand `op` in the descriptor of c"""
    return c[_GEMM_GS[op]], (c[_GEMM_LD[op]] if op in _GEMM_LD else c["N"] + 8)


def gemm_last_byte(c: dict, op: str) -> int:
    """byte offset, from the operand's base, one past the last element of `op` the descriptor of c makes a kernel touch"""
    G, rows, width = gemm_operand_shape(c, op)
    gstride, ldim = gemm_operand_strides(c, op)
    return 2 * ((G - 1) * gstride + (rows - 1) * ldim + width)


def gemm_far_layout(far: dict) -> dict:
    """element offsets of the operand bases of a far descriptor inside the arena: the operands with ordinary leading dimensions one behind the
    other (a group's share of each; group 1 repeats the pattern one group stride on), then those with the far leading dimension interleaved in
    the same rows, 1024 columns apart"""
    off, lay = ARENA_BASE, {}
    for op in GEMM_OPERANDS:
        G, rows, width = gemm_operand_shape(far, op)
        ldim = gemm_operand_strides(far, op)[1]
        if rows and ldim < (1 << 20):
            lay[op] = off + 64
            off += 64 + (rows * ldim + width + 2 * SENT_COLS + 63) // 64 * 64
    col = 0
    for op in GEMM_OPERANDS:
        if gemm_operand_shape(far, op)[1] and op not in lay:
            lay[op] = off + 64 + col
            col += 1024
    assert col <= 3 * 1024 < GEMM_LD_FAR and off - ARENA_BASE < (1 << 24)
    return lay


def gemm_far_view(arena: torch.Tensor, c: dict, lay: dict, op: str, extra: int = 0) -> torch.Tensor:
    """[groups, rows, width + extra] view of operand `op` of descriptor c at its place in the arena"""
    G, rows, width = gemm_operand_shape(c, op)
    gstride, ldim = gemm_operand_strides(c, op)
    assert lay[op] + (G - 1) * gstride + (rows - 1) * ldim + width + extra <= arena.numel(), "the view would leave the arena"
    return arena.as_strided((G, rows, width + extra), (gstride, ldim, 1), lay[op])


# ----------------------------------------------------------------------------------------------------------------------------------
# row-wise glue kernels: the last row of every strided operand past byte offset 2^32 from the operand's base
# ----------------------------------------------------------------------------------------------------------------------------------
def far_ld(rows: int, itemsize: int = 2) -> int:
    """the smallest leading dimension (a multiple of 8 elements) that puts row rows - 1 at or past byte offset 2^32"""
    return (-(-(1 << 32) // (itemsize * (rows - 1))) + 7) // 8 * 8


# (D, rows, rows per sample, x row map of the far launch or None): the two fast widths and a generic one with ldx = ldo = far_ld(rows), and
# one per kernel with compact rows and an x row map whose batch stride puts the last batch past 2^32 bytes
ADALN_FAR_CASES = [(1536, 300, 100, None), (3072, 200, 1, None), (520, 520, 130, None), (1536, 300, 100, "map"), (520, 390, 130, "map")]


def adaln_far_geometry(case):
    """-> dict(ldx, ldo, x_map) of the far launch of an ADALN_FAR_CASES entry (elements / rows)"""
    D, rows, rps, how = case
    if how is None:
        return dict(ldx=far_ld(rows), ldo=far_ld(rows), x_map=(0, 0))
    rpb, ldx = 100 if D == 1536 else 130, D + 8
    nb = -(-rows // rpb)
    return dict(ldx=ldx, ldo=far_ld(rows), x_map=(rpb, -(-(1 << 31) // (ldx * (nb - 1))) + 3))


GLUE_FAR_ROWS = {2: 520, 4: 300}          # rows of the strided operands, by element size: (rows - 1) far_ld(rows) elements reach 2^32 bytes
GLUE_FAR_D = 520


# ----------------------------------------------------------------------------------------------------------------------------------
# the 128^2 convolution kernel (and the fp32 twin) at real large-canvas layers: window checks against float64, and a bit-for-bit screen of
# every output element against the same kernel replayed on horizontal bands (each a small problem far below 2^31 bytes)
# ----------------------------------------------------------------------------------------------------------------------------------
CONV_BAND_ROWS = 256                     # output rows per band of the screen, and per seeded chunk of the data
# 4104 = 4096 + 8 rows: a 128-channel bf16 activation of 4096^2 ends exactly AT byte 2^32 (2^31 elements); eight more rows put the boundary inside
CONV_WINDOW_CASES = [
    dict(name="conv_in 64->128 at 4104x4096", H=4104, W=4096, Cin=64, Cout=128, stride=1, pad=1, res="none", f32=False, seed=6700),
    dict(name="resnet 128->128 at 4104x4096, R = out", H=4104, W=4096, Cin=128, Cout=128, stride=1, pad=1, res="alias", f32=False, seed=6701),
    dict(name="conv_out 128->8 at 4104x4096", H=4104, W=4096, Cin=128, Cout=8, stride=1, pad=1, res="none", f32=False, seed=6702),
    dict(name="downsample 128->128, 4104x4096 -> 2052x2048", H=4104, W=4096, Cin=128, Cout=128, stride=2, pad=0, res="none", f32=False, seed=6703),
    # the twin at Cout 8: its direct loop at Cout 128 (2.5 TFLOP of scalar FMAs per launch, by count) was NOT timed; x crosses 2^32 bytes, the output none
    dict(name="fp32 twin 128->8 at 2056x4096", H=2056, W=4096, Cin=128, Cout=8, stride=1, pad=1, res="none", f32=True, seed=6704),
]


def conv_window_out(c: dict):
    """(Ho, Wo) of a CONV_WINDOW_CASES entry, as unigen_amd/vae.py calls: 3 x 3 'same', or stride 2 without padding to half the size (the last
    tap of the last pixel falls off the bottom / right edge: the one-sided padding of Downsample2D)"""
    return (c["H"], c["W"]) if c["stride"] == 1 else (c["H"] // 2, c["W"] // 2)


def conv_band(c: dict, y0: int, y1: int) -> dict:
    """output rows [y0, y1) as a problem of its own: the input rows [x0, x1) it reads and the top padding left inside it"""
    first, last = y0 * c["stride"] - c["pad"], (y1 - 1) * c["stride"] - c["pad"] + 2          # 3 x 3 taps
    x0, x1 = max(first, 0), min(last + 1, c["H"])
    return dict(x0=x0, x1=x1, H=x1 - x0, pad_t=x0 - first, Ho=y1 - y0)


def conv_boundaries(c: dict) -> dict:
    """operand -> [(byte boundary, the first row that starts at or past it)] for the boundaries 2^31 and 2^32 that fall inside the operand"""
    es = 4 if c["f32"] else 2
    Ho, Wo = conv_window_out(c)
    out = {}
    for name, rows, rowbytes in (("x", c["H"], c["W"] * c["Cin"] * es), ("out", Ho, Wo * c["Cout"] * es)):
        out[name] = [(b, -(-b // rowbytes)) for b in (1 << 31, 1 << 32) if 0 < -(-b // rowbytes) < rows]
    return out


def conv_windows(c: dict) -> list:
    """the output-row windows [y0, y1) judged against float64: the first and last two rows, and two rows on either side of every byte
    boundary of the output and (through the rows that read them) of the input"""
    Ho, _ = conv_window_out(c)
    bd = conv_boundaries(c)
    at = [r for _, r in bd["out"]] + [r // c["stride"] for _, r in bd["x"]]
    wins = {(0, 2), (Ho - 2, Ho)} | {(max(r - 2, 0), min(r + 2, Ho)) for r in at if 0 < r < Ho}
    return sorted(wins)


# ----------------------------------------------------------------------------------------------------------------------------------
# GroupNorm (+ SiLU) on an activation of more than 2^31 elements: window checks. The statistics come from a float64 reduction by torch on
# the device, chunk by chunk (torch's reduction, not the kernel's); the windows from the float64 formula with those statistics.
# ----------------------------------------------------------------------------------------------------------------------------------
GN_CHUNK_ROWS = 1 << 18                  # rows per seeded chunk of the data and per step of the chunked reduction
GN_TAIL_SHIFT = 3.0                      # the last GN_TAIL_CHUNKS chunks are drawn around this mean instead of 0: the tail matters to the statistics
GN_TAIL_CHUNKS = 2
GN_WINDOW_ROWS = 256
GN_FAR_CASES = [
    dict(name="fast C128 G32 + SiLU", C=128, G=32, HW=4104 * 4096, silu=True, eps=1e-6, seed=6800),        # HW C = 2^31 + 2^22 elements
    dict(name="generic C64 G32", C=64, G=32, HW=8208 * 4096, silu=False, eps=1e-6, seed=6801),             # C = 64 is never the fast pair's
]


def gn_chunk_mean(c: dict, i: int) -> float:
    """the mean chunk i of a GN_FAR_CASES activation is drawn around"""
    n = -(-c["HW"] // GN_CHUNK_ROWS)
    return GN_TAIL_SHIFT if i >= n - GN_TAIL_CHUNKS else 0.0


def group_stats_chunked(x: torch.Tensor, G: int, chunk_rows: int, chunks=None):
    """x [HW, C] (one sample, any device and element type) -> (mean, biased variance) float64 [G], two passes of float64 sums over chunks of
    `chunk_rows` rows. chunks: the chunk indices to visit (default: all, once each) - the CPU companion drops or repeats the tail with it."""
    HW, C = x.shape
    ids = list(range(-(-HW // chunk_rows))) if chunks is None else list(chunks)
    part = lambda i: x[i * chunk_rows:(i + 1) * chunk_rows].to(torch.float64).reshape(-1, G, C // G)
    n = sum(min((i + 1) * chunk_rows, HW) - i * chunk_rows for i in ids) * (C // G)
    mean = sum(part(i).sum((0, 2)) for i in ids) / n
    var = sum(((part(i) - mean[None, :, None]) ** 2).sum((0, 2)) for i in ids) / n
    return mean, var


def groupnorm_with_stats(x, gamma, beta, G, eps, silu, mean, var):
    """vae_kernel_ref.groupnorm on rows x [B, rows, C] of a larger sample whose statistics (mean, var: float64 [G]) are given -> (truth, variant)"""
    F64, F32 = torch.float64, torch.float32
    B, R, C = x.shape
    mean, var = mean.reshape(1, 1, G, 1).cpu(), var.reshape(1, 1, G, 1).cpu()
    rstd = torch.rsqrt(var + VR.f32(eps))
    xg = x.to(F64).reshape(B, R, G, C // G)
    y = ((xg - mean) * rstd).reshape(B, R, C) * gamma.to(F64) + beta.to(F64)
    truth = y * torch.sigmoid(y) if silu else y
    v = ((xg.to(F32) - mean.to(F32)) * rstd.to(F32)).reshape(B, R, C) * gamma.to(F32) + beta.to(F32)
    v = v.to(torch.bfloat16).to(F32)
    if silu:
        v = (v / (1.0 + torch.exp(-v))).to(torch.bfloat16).to(F32)
    return truth, v.to(F64)


def gn_windows(c: dict) -> list:
    """row windows [r0, r1) of x and out (same layout, bf16): the first and last GN_WINDOW_ROWS rows and as many on either side of byte offsets
    2^31 and 2^32"""
    rowbytes, HW, w = 2 * c["C"], c["HW"], GN_WINDOW_ROWS
    at = [b // rowbytes for b in (1 << 31, 1 << 32) if 0 < b // rowbytes < HW]
    return sorted({(0, w), (HW - w, HW)} | {(r - w, r + w) for r in at})


# ----------------------------------------------------------------------------------------------------------------------------------
# more row-wise kernels with strided operands past byte offset 2^32: ug_qk_rmsnorm_rope (ld; batch_stride_rows), ug_small_linear_bf16
# (x, residual, out and W strides), ug_qk_rmsnorm_rope_bwd and ug_adaln_modulate_bwd (x, dy; the scale's row stride)
# ----------------------------------------------------------------------------------------------------------------------------------
QK_FAR = dict(heads=2, dh=128, batches=3, rpb=100, width=2 * 2 * 128 + SENT_COLS)        # q | k | sentinels in one row


def qk_far_geometries() -> dict:
    """name -> (ld, batch_stride_rows) of the two far launches of ug_qk_rmsnorm_rope"""
    rows, w = QK_FAR["batches"] * QK_FAR["rpb"], QK_FAR["width"]
    return dict(ld=(far_ld(rows), QK_FAR["rpb"]), batch_stride=(w, -(-(1 << 31) // (w * (QK_FAR["batches"] - 1))) + 5))


SMALL_LINEAR_FAR = (48, 520, 520, True, True, True)      # M (three launches of 16 rows), N, K, SiLU, bias, residual: a tests/test_fuzz_gemm_gpu.py case tuple
ADALN_BWD_FAR = dict(D=1536, rps=100, samples=3)
