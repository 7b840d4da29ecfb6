"""CPU float64 reference of the head-width-512 flash attention forward (csrc/attn_wide.hip: ug_flash_attn_fwd_wide and its fp32 twin), and the case
list tests/test_attn_wide_gpu.py runs and tests/test_attn_wide_ref_cpu.py checks on the host.

    reference(q, k, v, scale) -> dict(O=..., O_v=...)
        O    exact softmax attention of the operands as the kernel sees them (bf16 values widened to float64)
        O_v  the rounding-point variant along flash_attn_wide_kernel's own online-softmax trajectory: per row and KV_TILE keys the reference point
             becomes the tile's maximum in the first tile and later only where that maximum exceeds it by more than LAZY in log2 units
             (`up = (tmax - m_run) * c > 8.0f`), p = 2^(c s - m), bf16(p) is the P.V operand, the accumulator and l are rescaled by 2^(m_old - m_new),
             l adds the fp32 p, the output is bf16(acc / l). It is bwd_ref.forward_lazy at the wide kernel's tile length (32 keys, not 64).
    slipped(q, k, v, scale, slip) -> the same variant with one deliberate mistake (SLIPS): the host tests show that the GPU bounds catch each.

The peaked-row regimes are bwd_ref.attention_regime's, which is general in the head width (its ramps and spikes are laid out on 64-key tiles: two of
this kernel's tiles, so a "rising" row moves its reference point at every second tile and a "near_threshold" spike sits inside a later tile)."""
import math

import torch

from tests import bwd_ref as BR

F64 = torch.float64
DH = 512
KV_TILE = 32                 # keys per tile of flash_attn_wide_kernel (WKV)
LAZY = 8.0                   # its lazy-reference-point threshold, in log2 units of c S
FLOOR = 2.0 ** -9            # the project's floor under 1.5 x the variant's own error (docs/PARITY_TOLERANCES.md, "Attention regimes sweep")
ROW_BOUND = 4e-3             # the project's attention row: what err(O_v) itself has to stay under

# (B, H, Lq, Lkv): the smallest shapes at which each mechanism can go wrong
SHAPES = [(1, 1, 1, 1),            # single element
          (1, 1, 31, 33),          # under one 128-row query tile, one key past a 32-key tile
          (1, 1, 64, 64),          # whole tiles only
          (1, 1, 65, 65),          # one tile plus one element
          (2, 1, 100, 333),        # ragged, batch stride != L x row stride
          (1, 2, 257, 520),        # two heads: head offset head * 512; three query tiles, the last one row deep
          (1, 1, 1024, 1024),      # many tiles
          (1, 1, 2125, 1100)]      # several workgroups per round, both tails ragged
REGIMES = ("rising", "near_threshold", "one_key")
REGIME_SHAPES = [(2, 1, 100, 333), (1, 2, 257, 520)]
SCALES = (DH ** -0.5, 4 * DH ** -0.5, DH ** -0.5 / 4)
SLIPS = ("no_rescale", "tail_unmasked", "scale_128", "drop_partial_tile")


def case_ids():
    ids = ["gaussian-%dx%dx%dx%d" % s for s in SHAPES]
    ids += ["%s-%dx%dx%dx%d-s%d" % ((r,) + s + (si,)) for r in REGIMES for s in REGIME_SHAPES for si in range(len(SCALES))]
    return ids


def case_spec(case_id):
    parts = case_id.split("-")
    B, H, Lq, Lkv = (int(x) for x in parts[1].split("x"))
    si = int(parts[2][1:]) if len(parts) > 2 else 0
    return dict(id=case_id, regime=parts[0], B=B, H=H, Lq=Lq, Lkv=Lkv, scale=SCALES[si], seed=4100 + case_ids().index(case_id))


_DATA = {}


def case_data(case_id):
    """-> dict(q [B, H, Lq, 512], k, v [B, H, Lkv, 512] in bf16, rows: the query rows the regime acts on, scale, ...); computed once per process"""
    if case_id not in _DATA:
        s = case_spec(case_id)
        g = torch.Generator().manual_seed(s["seed"])
        if s["regime"] == "gaussian":
            rn = lambda L_: torch.randn(s["B"], s["H"], L_, DH, generator=g).to(torch.bfloat16)
            d = dict(q=rn(s["Lq"]), k=rn(s["Lkv"]), v=rn(s["Lkv"]), rows=torch.arange(0))
        else:
            d = BR.attention_regime(g, s["regime"], DH, s["B"], s["H"], s["Lq"], s["Lkv"], s["scale"])
        _DATA[case_id] = dict(s, q=d["q"], k=d["k"], v=d["v"], rows=d["rows"])
    return _DATA[case_id]


_REF = {}


def case_reference(case_id):
    """reference() of a case, computed once per process and shared by the tests (treat it as read-only)"""
    if case_id not in _REF:
        d = case_data(case_id)
        _REF[case_id] = reference(d["q"], d["k"], d["v"], d["scale"])
    return _REF[case_id]


def _trajectory(cs, v, tile, lazy, no_rescale=False):
    """the kernel's online softmax over cs = c S [..., Lq, n] and v [..., n, dh] (n: however many keys the caller lets the kernel see)"""
    lead = cs.shape[:-1]
    m = torch.full(lead, -math.inf, dtype=F64)
    l = torch.zeros(lead, dtype=F64)
    acc = torch.zeros(*lead, v.shape[-1], dtype=F64)
    for t, k0 in enumerate(range(0, cs.shape[-1], tile)):
        ct = cs[..., k0:k0 + tile]
        tmax = ct.amax(-1)
        up = (tmax - m) > lazy if t else torch.ones(lead, dtype=torch.bool)
        m_new = torch.where(up, tmax, m)
        alpha = torch.where(up, torch.exp2(m - m_new), torch.ones_like(m))
        p = torch.exp2(ct - m_new[..., None])
        acc = (acc if no_rescale else acc * alpha[..., None]) + BR.bf16(p) @ v[..., k0:k0 + tile, :]
        l = l * alpha + p.sum(-1)
        m = m_new
    return BR.bf16(acc / l[..., None])


def reference(q, k, v, scale, tile=KV_TILE, lazy=LAZY):
    q, k, v = (t.to(F64) for t in (q, k, v))
    cs = (scale * BR.LOG2E) * (q @ k.transpose(-1, -2))
    p = torch.exp2(cs - cs.amax(-1, keepdim=True))
    return dict(O=(p / p.sum(-1, keepdim=True)) @ v, O_v=_trajectory(cs, v, tile, lazy))


def slipped(q, k, v, scale, slip, tile=KV_TILE, lazy=LAZY, seed=0):
    """O_v with one mistake a kernel of this kind can make:
      no_rescale         the running O is not rescaled when a row's reference point rises (l is)
      tail_unmasked      the ragged key tail is not masked: the last tile is filled up with finite garbage keys and values, and they count
      scale_128          128^-0.5 in place of 512^-0.5 (twice the scale)
      drop_partial_tile  the last, partial key tile is never visited (no whole tile at all: nothing is written, NaN)"""
    assert slip in SLIPS
    q, k, v = (t.to(F64) for t in (q, k, v))
    Lkv = k.shape[-2]
    if slip == "scale_128":
        scale = scale * 2.0
    elif slip == "tail_unmasked" and Lkv % tile:
        g = torch.Generator().manual_seed(seed)
        pad = tile - Lkv % tile
        k = torch.cat([k, BR.bf16(torch.randn(*k.shape[:-2], pad, k.shape[-1], generator=g, dtype=F64))], -2)
        v = torch.cat([v, BR.bf16(torch.randn(*v.shape[:-2], pad, v.shape[-1], generator=g, dtype=F64))], -2)
    elif slip == "drop_partial_tile" and Lkv % tile:
        if Lkv < tile:
            return torch.full((*q.shape[:-1], v.shape[-1]), float("nan"), dtype=F64)
        k, v = k[..., :Lkv // tile * tile, :], v[..., :Lkv // tile * tile, :]
    cs = (scale * BR.LOG2E) * (q @ k.transpose(-1, -2))
    return _trajectory(cs, v, tile, lazy, no_rescale=slip == "no_rescale")


def bounds(ref, rows=None):
    """(total, worst row) bounds of the bf16 kernel against ref['O']: max(1.5 x err(O_v), 2^-9) each; rows: on those query rows alone"""
    O, Ov = ref["O"], ref["O_v"]
    if rows is not None:
        O, Ov = O[..., rows, :], Ov[..., rows, :]
    e = BR.err(Ov, O)
    return max(1.5 * e[0], FLOOR), max(1.5 * e[1], FLOOR)
