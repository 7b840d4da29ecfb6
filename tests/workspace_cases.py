"""Data of tests/test_workspace_gpu.py (checked without a device by tests/test_workspace_cases_cpu.py): the GEMM launch sequence whose split-K
launches share one workspace, and for every other workspace-taking entry point two shapes with different partial counts.

GEMM_SEQUENCE: cases of tests/test_fuzz_gemm_gpu.GEMM_CASES by name (their buffer geometry and operand builders are reused), in launch order. At
256 CUs their (K-slices, padded tail tiles) are (8, 24) (5, 48) (3, 72) (1, 0) (8, 24) (8, 8): every launch meets slabs and tickets that a
launch of a different slice count or tile count left behind, in this order, in reverse, and when the sequence repeats.

A launch of path (tile, rounds, nsl, rem8, wide) may touch the arrival tickets (bytes [0, 4096)) and the slabs of its own K-slices, bytes
[4096, 4096 + rem8 * nsl * 65536 * 4); an unsplit launch touches nothing.

WORKSPACES: entry point -> dict(unit = the alignment unit of its workspace (bytes; the undersized call passes the reported size minus one unit),
dtypes, a, b = two shapes (keyword arguments of the runner in the GPU test), bytes = the size formula of include/unigen_hip.h restated).
Shape `a` is the smallest that makes more than one partial / split / chunk, `b` has a different partial count."""
from tests.test_fuzz_gemm_gpu import GEMM_CASES

GEMM_SEQUENCE_NAMES = [
    "small-M 24 tiles K 12288, res_gate",
    "small-M 48 tiles ragged M, no bias",
    "small-M 72 tiles K 15360, A row map, res_gate",
    "narrow epilogue: ldc % 8 == 4",                       # unsplit 256^2: 256 tiles, one full round
    "small-M 24 tiles K 6144",
    "tail 5 of 261, gelu",
]
_BY_NAME = {c["name"]: i for i, c in enumerate(GEMM_CASES)}
GEMM_SEQUENCE = [_BY_NAME[n] for n in GEMM_SEQUENCE_NAMES]          # indices into GEMM_CASES (the index seeds the operands, as in the sweep)
SMALL_M = _BY_NAME["small-M 24 tiles K 12288, res_gate"]            # the case of the ops.gemm / two-stream product-path test
TICKET_BYTES = 4096
SLAB_BYTES = 65536 * 4
GEMM_WORKSPACE_BYTES = TICKET_BYTES + 256 * SLAB_BYTES              # ug_gemm_workspace_bytes()


def gemm_touched_bytes(path):
    """bytes from the start of the workspace that a launch of this path may write"""
    _, _, nsl, rem8, _ = path
    return TICKET_BYTES + (rem8 * nsl * SLAB_BYTES if nsl > 1 else 0)


def slice_tail(path):
    return path[2], path[3]


def _cdiv(a, b):
    return (a + b - 1) // b


def _pad64(n):
    return _cdiv(n, 64) * 64


def _up256(n):
    return _cdiv(n, 256) * 256


def groupnorm_bytes(B, HW, C, G):
    return B * _cdiv(HW, 64) * G * 2 * 8 + B * G * 2 * 4 + 64


def colsum_bytes(rows, cols, rpg, **_):
    return (rows // rpg) * _cdiv(rpg, 128) * cols * 4


def lora_wgrad_splits(M, R, J):
    nblk, tiles = _cdiv(M, 64), _cdiv(J, 128) * (R // 64)
    want = max(1, min(_cdiv(512, tiles), _cdiv(nblk, 4)))
    return _cdiv(nblk, _cdiv(nblk, want))


def lora_wgrad_bytes(M, R, J):
    return lora_wgrad_splits(M, R, J) * R * J * 4


def flash_attn_bwd_bytes(B, H, Lq, **_):
    return 2 * B * H * _pad64(Lq) * 4


def grad_sumsq_chunks(numels):
    return sum(_cdiv(n, 65536) for n, _ in numels)


def grad_sumsq_bytes(numels):
    return max(grad_sumsq_chunks(numels), 1) * 8


def canny_bytes(B, H, W, **_):
    n = B * H * W
    return 2 * _up256(2 * n) + _up256(4 * n) + _up256(n) + 256


def blur_bytes(B, H, W, C, **_):
    return 2 * _up256(B * H * W * C)


WORKSPACES = {
    # GroupNorm partials are per 64 pixels: HW = 65 makes two. C = 64 runs the generic kernels, C = 128 the 256-pixel fast pair in bf16
    "ug_groupnorm_nhwc": dict(unit=8, dtypes=("bf16", "f32"), bytes=groupnorm_bytes, a=dict(B=1, HW=65, C=64, G=32), b=dict(B=2, HW=200, C=64, G=32)),
    "ug_groupnorm_nhwc/fast": dict(unit=8, dtypes=("bf16",), bytes=groupnorm_bytes, a=dict(B=1, HW=257, C=128, G=32), b=dict(B=2, HW=520, C=128, G=32)),
    # colsum chunks are 128 rows of a group: 129 rows in one group make two; (300, 520, 100) of the backward sweep: three groups of one chunk
    "ug_colsum": dict(unit=4, dtypes=("bf16", "f32"), bytes=colsum_bytes, a=dict(rows=129, cols=8, rpg=129, with_b=False),
                      b=dict(rows=300, cols=520, rpg=100, with_b=True)),
    # a split of ug_lora_wgrad is at least 4 blocks of 64 rows: M = 257 (5 blocks) makes two; (1000, 128, 1536) of its sweep makes four
    "ug_lora_wgrad": dict(unit=16, dtypes=("bf16", "f32"), bytes=lora_wgrad_bytes, a=dict(M=257, R=64, J=64), b=dict(M=1000, R=128, J=1536)),
    # statistics per (batch, head, query), rows padded to 64: Lq = 333 is no multiple of 64; both head widths, lse_in given and NULL
    "ug_flash_attn_bwd/64": dict(unit=16, dtypes=("bf16",), bytes=flash_attn_bwd_bytes, a=dict(B=2, H=1, Lq=65, Lkv=129, dh=64),
                                 b=dict(B=1, H=2, Lq=333, Lkv=520, dh=64)),
    "ug_flash_attn_bwd/128": dict(unit=16, dtypes=("bf16",), bytes=flash_attn_bwd_bytes, a=dict(B=2, H=1, Lq=65, Lkv=129, dh=128),
                                  b=dict(B=1, H=2, Lq=333, Lkv=520, dh=128)),
    # the pair-scheme dQ (head width 128, Lq >= 2048) next to a shape below the switch
    "ug_flash_attn_bwd/pair_dq": dict(unit=16, dtypes=("bf16",), bytes=flash_attn_bwd_bytes, a=dict(B=1, H=1, Lq=333, Lkv=520, dh=128),
                                      b=dict(B=1, H=1, Lq=2049, Lkv=520, dh=128)),
    # one fp64 partial per 65536-element chunk: 65537 elements make two; three tensors of both dtypes make six
    "ug_grad_sumsq": dict(unit=8, dtypes=("mixed",), bytes=grad_sumsq_bytes, a=dict(numels=((65537, "f32"),)),
                          b=dict(numels=((100, "bf16"), (200000, "f32"), (65536, "bf16")))),
    "ug_canny_u8": dict(unit=16, dtypes=("u8",), bytes=canny_bytes, a=dict(B=1, H=40, W=70, C=1), b=dict(B=2, H=67, W=131, C=3)),
    # fuse = 0: one launch per pass, the launches alternate between the workspace's two images; fuse = 1: one launch per axis
    "ug_img_box_blur_u8": dict(unit=16, dtypes=("u8",), bytes=blur_bytes, a=dict(B=1, H=40, W=70, C=1, radius=2.0, passes=3, fuse=0),
                               b=dict(B=2, H=67, W=131, C=3, radius=1.5, passes=3, fuse=1)),
}

# partial-sum outputs the caller reduces: (rows, rows_per_sample, D) / (rows, heads, dh) / (S, D, E). The first of each has one partial row; the
# others have a row count that is no multiple of the per-partial share (rows = 777, rows per sample 7 and 100 of the backward sweep), and
# (6000, 2000): three samples of 341 partials of 6 rows, the last 7 of each sample empty
ADALN_BWD_PARTIALS = [(1, 1, 64), (777, 7, 520), (300, 100, 64), (6000, 2000, 64)]
QK_BWD_PARTIALS = [(1, 1, 64), (777, 3, 128), (100, 24, 64), (4099, 3, 64)]           # blocks of 4 (row, head) vectors, at most 2048 partial rows
MOE_GATE_BWD_PARTIALS = [(1, 64, 2), (777, 520, 6), (129, 64, 16)]                   # slices of 128 tokens


def adaln_bwd_partials(rows, rps):
    return max(1, min(1024 // max(rows // rps, 1), _cdiv(rps, 4)))


def qk_bwd_partials(rows, heads):
    return max(1, min(2048, _cdiv(rows * heads, 4)))


def moe_gate_bwd_slices(S):
    return _cdiv(S, 128)
