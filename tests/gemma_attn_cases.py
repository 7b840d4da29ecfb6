"""The case grid of the head-width-256 soft-cap attention sweep (attn_plain_kernel<256, 32, false, true, CAP, true> behind ug_flash_attn_fwd_softcap and
flash_attn_f32_kernel<256, 4, false, true> behind ug_flash_attn_fwd_softcap_f32): tests/test_fuzz_gemma_gpu.py runs every case on the device,
tests/test_gemma_attn_cases_cpu.py checks on the host what each case promises, computes the bounds the device test uses from the references alone and
shows that every mutant of gemma_ref.attention is caught by some case. Host only: no GPU import. Operands are built on demand (case_data), never at
import; they are bf16-representable float64.

GEOMETRY cases put the window, the key lengths and the sequence length on the kernel's edges: 32-key tiles (KT), 128 query rows per workgroup (AQ),
the workgroup's first tile klo = max(0, Q0 - window + 1), a wave's tile skip k0 + KT - 1 <= q0 - window, the key mask key <= qrow - window, kv_len
clamped to [0, L], window >= L folded to none. Operands are Gaussian (q, k at standard deviation 2, v at 1, independent K/V head draws); V carries 1e4
from kv_len[b] on, which no row may see. Not a Cartesian product: a hand-picked table in which every value of GEO_L, GEO_WINDOWS, GEO_KV and LAYOUTS
occurs (tests/test_gemma_attn_cases_cpu.py asserts the coverage), each of the windows 31 / 32 / 33 / 127 / 128 / 129 with lengths more than a tile
beyond it, each kv_len edge once without a window and once with one of a tile or more, and three lists that leave a whole workgroup without a live key.

REGIME cases shape the scores. Amplitudes are in log2 units of the final (capped) score, bwd_ref's BACKGROUND, RAMP and SPIKE; bwd_ref.attention_regime
itself assumes 64-key tiles and no mask, so what is needed is restated here for a causal launch on 32-key tiles. Background q is drawn at standard
deviation BACKGROUND / (c sqrt(dh)), c = scale log2(e), against unit k, both without their components along the orthonormal directions u_i that carry
the regime: a chosen row gains A u_i and a key b u_i, so exactly that pair's pre-cap score gains scale A b, which is cap atanh(target / cap) for a
target under a cap.
  rising / falling    rows 0, 3, 6, ... (every wave of a workgroup, every lane): every key gains +- RAMP x (its 32-key tile's index, centred), so a
                      chosen row's tile maximum gains / loses RAMP in every live tile up to its diagonal
  spike_diag          the same rows, one direction each: the row's own key is SPIKE above all others
  spike_window_first  windows 32, 33, 97: rows window + 30 + j (window + 5), the first of which has its window's first key as the LAST key of a tile:
                      key qrow - window + 1 is at SPIKE and dominates; key qrow - window, which is hidden, is at 2 SPIKE and carries a V of 1e4. The
                      rows that legitimately see such a key are "dirty" and judged apart
  spike_kvlen_last    rows 0, 3, 6, ...: key kv_len - 1 is at SPIKE; key kv_len, hidden, at 2 SPIKE with a V of 1e4
  saturated           caps 4 and 50: rows and keys carry signs, scale q.k = +- 64 cap for seven keys of eight (the eighth: background), so e^(2y) is
                      exactly 0 or inf in the kernel and whole runs of keys tie at exactly +cap and -cap
"""
import functools
import math
import zlib

import torch

from tests import gemma_ref as R
from tests.bwd_ref import BACKGROUND, RAMP, SPIKE
from tests.text_ref import _rel_l2, worst_row

F32, F64 = torch.float32, torch.float64
DH, SCALE = 256, 256 ** -0.5
KT, AQ = 32, 128
LOG2E = 1.4426950408889634
BIG_V = 9984.0                                        # 1e4 rounded to bf16
CASE_CAP = 2_000_000                                  # B H L^2, the cap of attn_regime_cases
FLOOR = 2.0 ** -9
LAYOUTS = ((4, 2), (2, 2), (2, 1), (3, 1), (4, 1))
CAPS = (0.0, 50.0, 4.0)
GEO_L = (1, 32, 33, 96, 128, 129, 160, 257, 300)
GEO_WINDOWS = (0, 1, 2, 31, 32, 33, 64, 97, 127, 128, 129, "L-1", "L", "L+5", 4096)
GEO_KV = (0, 1, 31, 32, 33, 127, 128, 129, "L-1", "L")
EDGE_WINDOWS = (31, 32, 33, 127, 128, 129)
REGIMES = ("rising", "falling", "spike_diag", "spike_window_first", "spike_kvlen_last", "saturated")
SATURATION = 64.0                                     # saturated: |scale q.k| / cap of a signed pair
SPIKE_CLEAR, RAMP_CLEAR = 2.5, 2.5                    # the background (standard deviation BACKGROUND = 0.3) stays within 4 deviations = 1.2 on either side

_L = "L"
# (L, window, kv_len list or None); "L-1", "L", "L+5" are resolved against the row's L
_GEOMETRY = (
    # the windows on a tile / workgroup edge, with lengths more than a tile beyond them
    (96, 31, None), (129, 31, [_L, 33]), (300, 31, None), (96, 32, ["L-1", _L]), (129, 32, None), (300, 32, [_L, 127]),
    (96, 33, None), (129, 33, [128, _L]), (300, 33, None), (257, 127, None), (300, 127, [_L, 129, 128]),
    (257, 128, ["L-1", _L]), (300, 128, None), (257, 129, None), (300, 129, ["L-1", _L]),
    # every kv_len edge without a window ...
    (160, 0, [0, _L]), (300, 0, [_L, 1]), (257, 0, [31, 32, 33]), (300, 0, [127, 128, 129]), (160, 0, ["L-1", _L, 1]), (129, 0, [128, _L, 0]),
    # ... and with one of a tile or more
    (160, 32, [0, _L]), (300, 64, [_L, 1]), (257, 33, [31, 32, 33]), (300, 97, [127, 128, 129]), (160, 64, ["L-1", _L, 1]), (129, 97, [128, _L, 0]),
    # kv_len + window below 128 with L above: the second workgroup of that sample has no live key
    (300, 32, [_L, 33]), (257, 64, [33, _L, 1]), (160, 2, [31, _L]),
    # the remaining lengths and windows
    (1, 0, None), (1, 1, [1, 0]), (1, "L+5", [1, 1]),
    (32, 1, None), (32, 2, [_L, 31]), (32, 31, [_L, 1]), (32, 32, None), (32, "L+5", [31, _L]),
    (33, 32, [_L, 32]), (33, 33, None), (33, 1, [_L, 31, 0]), (33, 4096, [32, _L]),
    (96, 64, [33, _L]), (96, 97, None), (96, "L-1", [_L, 31]),
    (128, 127, None), (128, 128, [_L, 127]), (128, 129, None), (128, 64, [127, _L, 0]), (128, 97, [_L, 33]),
    (129, 128, [_L, 1]), (129, "L", None),
    (160, 97, None), (160, "L-1", [_L, 129]), (160, 127, [_L, 33]),
    (257, "L+5", None), (257, 4096, [_L, 129]),
    (300, "L-1", None), (300, "L", [_L, "L-1"]), (300, 4096, [_L, 128]), (300, 1, [_L, 129]), (300, 64, None),
)
# (regime, L, cap, window, kv_len)
_REGIME_TABLE = (
    ("rising", 96, 0.0, 0, None), ("rising", 160, 50.0, 0, None), ("rising", 300, 0.0, 0, None), ("rising", 300, 50.0, 0, None),
    ("falling", 96, 50.0, 0, None), ("falling", 160, 0.0, 0, None), ("falling", 300, 0.0, 0, None), ("falling", 300, 50.0, 0, None),
    ("spike_diag", 96, 0.0, 0, None), ("spike_diag", 96, 50.0, 0, None), ("spike_diag", 160, 0.0, 0, None), ("spike_diag", 160, 50.0, 0, None),
    ("spike_diag", 300, 0.0, 0, None), ("spike_diag", 300, 50.0, 0, None),
    ("spike_window_first", 96, 0.0, 32, None), ("spike_window_first", 160, 50.0, 32, None), ("spike_window_first", 300, 0.0, 32, None),
    ("spike_window_first", 96, 50.0, 33, None), ("spike_window_first", 160, 0.0, 33, None), ("spike_window_first", 300, 50.0, 33, None),
    ("spike_window_first", 160, 50.0, 97, None), ("spike_window_first", 300, 0.0, 97, None),
    ("spike_kvlen_last", 96, 0.0, 0, [89, 33]), ("spike_kvlen_last", 160, 50.0, 0, [129, 153]), ("spike_kvlen_last", 300, 0.0, 0, [293, 128]),
    ("saturated", 96, 4.0, 0, None), ("saturated", 160, 4.0, 33, None), ("saturated", 300, 4.0, 0, None),
    ("saturated", 96, 50.0, 0, None), ("saturated", 160, 50.0, 0, None), ("saturated", 300, 50.0, 97, None),
)


def _resolve(x, L):
    return {"L-1": L - 1, "L": L, "L+5": L + 5}[x] if isinstance(x, str) else x


def _name(x):
    return {"L-1": "Lm1", "L+5": "Lp5"}.get(x, str(x))


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of case dicts (shapes and parameters, no data): id, kind ('geometry' or a regime), B, L, H, KV, cap, window, kv_len (list or None), and
    for the geometry rows the table's own spelling of the window and the key lengths (window_spec, kv_spec)"""
    out = []
    for i, (L, w, kv) in enumerate(_GEOMETRY):
        (H, KV), cap = LAYOUTS[i % len(LAYOUTS)], CAPS[i % len(CAPS)]
        B = len(kv) if kv else 2
        cid = f"geo{i:02d}-L{L}-w{_name(w)}-kv{'none' if kv is None else '_'.join(_name(n) for n in kv)}-h{H}kv{KV}-cap{cap:g}"
        out.append(dict(id=cid, kind="geometry", B=B, L=L, H=H, KV=KV, cap=cap, window=_resolve(w, L), kv_len=None if kv is None else [_resolve(n, L) for n in kv],
                        window_spec=w, kv_spec=kv))
    for i, (regime, L, cap, w, kv) in enumerate(_REGIME_TABLE):
        H, KV = LAYOUTS[i % len(LAYOUTS)]
        cid = f"{regime}-L{L}-cap{cap:g}-w{w}-h{H}kv{KV}"
        out.append(dict(id=cid, kind=regime, B=2, L=L, H=H, KV=KV, cap=cap, window=w, kv_len=kv))
    assert len({c["id"] for c in out}) == len(out) and all(c["B"] * c["H"] * c["L"] ** 2 < CASE_CAP for c in out)
    return tuple(out)


def case_ids(kind=None):
    return [c["id"] for c in cases() if kind is None or (c["kind"] != "geometry" if kind == "regime" else c["kind"] == kind)]


def case(case_id):
    return next(c for c in cases() if c["id"] == case_id)


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _pre(target_log2: float, cap: float) -> float:
    """the pre-cap natural-unit score whose capped value is target_log2 in log2 units"""
    t = target_log2 / LOG2E
    if not cap:
        return t
    assert abs(t) < 0.9 * cap, (target_log2, cap)
    return cap * math.atanh(t / cap)


def regime_rows(c):
    """the query rows the regime acts on (the same in every sample and head)"""
    L, w = c["L"], c["window"]
    if c["kind"] == "spike_window_first":
        return list(range(w + 30, L, w + 5))
    if c["kind"] == "saturated":
        return list(range(L))
    return list(range(0, L, 3))


def _geometry_data(c, g):
    B, L, H, KV = c["B"], c["L"], c["H"], c["KV"]
    q = torch.randn(B, L, H, DH, generator=g, dtype=F64) * 2.0
    k = torch.randn(B, L, KV, DH, generator=g, dtype=F64) * 2.0
    v = torch.randn(B, L, KV, DH, generator=g, dtype=F64)
    planted = torch.zeros(B, L, dtype=torch.bool)
    if c["kv_len"] is not None:
        for b, n in enumerate(c["kv_len"]):
            planted[b, n:] = True
    return dict(q=q, k=k, v=v, planted=planted, rows=torch.arange(0), row_key=torch.zeros(B, 0, dtype=torch.int64))


def _regime_data(c, g):
    B, L, H, KV, cap, w, regime = c["B"], c["L"], c["H"], c["KV"], c["cap"], c["window"], c["kind"]
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=F64)
    rows = regime_rows(c)
    per_row = regime in ("spike_diag", "spike_window_first")
    U = torch.linalg.qr(rn(DH, len(rows) if per_row else 1))[0]         # [dh, n] orthonormal columns
    off = lambda t: t - (t @ U) @ U.T
    q = off(rn(B, L, H, DH) * (BACKGROUND / (SCALE * LOG2E * math.sqrt(DH))))
    k, v = off(rn(B, L, KV, DH)), rn(B, L, KV, DH)
    planted = torch.zeros(B, L, dtype=torch.bool)
    row_key = torch.full((B, len(rows)), -1, dtype=torch.int64)
    A = 4.0                                                              # a chosen row's amplitude; the key's is pre-cap score / (scale A)
    amp = lambda target: _pre(target, cap) / (SCALE * A)
    rt = torch.tensor(rows)
    if regime in ("rising", "falling"):
        nt = (L + KT - 1) // KT
        sign = 1.0 if regime == "rising" else -1.0
        per_tile = torch.tensor([amp(sign * RAMP * (t - (nt - 1) / 2)) for t in range(nt)], dtype=F64)
        k = k + per_tile[torch.arange(L) // KT][None, :, None, None] * U[:, 0]
        q[:, rt] += A * U[:, 0]
    elif regime == "spike_diag":
        for i, r in enumerate(rows):
            q[:, r] += A * U[:, i]
            k[:, r] += amp(SPIKE) * U[:, i]
        row_key[:] = rt
    elif regime == "spike_window_first":
        for i, r in enumerate(rows):
            q[:, r] += A * U[:, i]
            k[:, r - w + 1] += amp(SPIKE) * U[:, i]
            k[:, r - w] += amp(2 * SPIKE) * U[:, i]
            v[:, r - w] = BIG_V
            planted[:, r - w] = True
        row_key[:] = rt - w + 1
    elif regime == "spike_kvlen_last":
        q[:, rt] += A * U[:, 0]
        for b, n in enumerate(c["kv_len"]):
            k[b, n - 1] += amp(SPIKE) * U[:, 0]
            k[b, n] += amp(2 * SPIKE) * U[:, 0]
            v[b, n] = BIG_V
            planted[b, n] = True
            row_key[b] = torch.where(rt >= n - 1, torch.full_like(rt, n - 1), torch.full_like(rt, -1))
    else:
        assert regime == "saturated" and cap
        a = math.sqrt(SATURATION * cap / SCALE)
        sq = torch.where(torch.rand(B, L, H, generator=g) < 0.5, -1.0, 1.0).to(F64)
        u = torch.rand(B, L, KV, generator=g)
        sk = torch.where(u < 0.125, 0.0, torch.where(u < 0.5625, -1.0, 1.0)).to(F64)
        q = q + (a * sq)[..., None] * U[:, 0]
        k = k + (a * sk)[..., None] * U[:, 0]
    return dict(q=q, k=k, v=v, planted=planted, rows=rt, row_key=row_key)


@functools.lru_cache(maxsize=4)
def case_data(case_id):
    """-> dict: q [B, L, H, 256], k, v [B, L, KV, 256] float64 holding bf16 values; planted bool [B, L]: the keys whose V is 1e4; rows: the chosen query
    rows; row_key [B, len(rows)]: each chosen row's dominant key (-1: none)"""
    c = case(case_id)
    g = torch.Generator().manual_seed(zlib.crc32(case_id.encode()))
    d = _geometry_data(c, g) if c["kind"] == "geometry" else _regime_data(c, g)
    d["q"], d["k"], d["v"] = R.bf(d["q"]), R.bf(d["k"]), R.bf(d["v"])
    d["v"][d["planted"]] = BIG_V
    return d


def scores(c, d):
    """-> (pre-cap scale q.k, final capped scores in log2 units) [B, H, L, L] in float64, no mask"""
    g = c["H"] // c["KV"]
    s = torch.einsum("bqhd,bkhd->bhqk", d["q"], d["k"].repeat_interleave(g, dim=2)) * SCALE
    return s, (torch.tanh(s / c["cap"]) * c["cap"] if c["cap"] else s) * LOG2E


# ---- references, row groups, bounds ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def refs(case_id):
    """-> dict: truth (float64), variant (the rounding points of the bf16 kernel), host32 (the float32 host evaluation; None without a cap), live
    [B, L, L], dead [B, L] (no live key: the output is defined as zero), dirty [B, L] (the row legitimately sees a V of 1e4), clean (neither)"""
    c, d = case(case_id), case_data(case_id)
    args = (d["q"], d["k"], d["v"], SCALE, c["cap"], c["window"], c["kv_len"])
    live = R.live_keys(c["L"], c["window"], c["kv_len"], c["B"])
    dead = ~live.any(-1)
    dirty = (live & d["planted"][:, None, :]).any(-1)
    return dict(truth=R.attention(*args), variant=R.attention(*args, rnd=R.bf), host32=R.attention(*args, dtype=F32).to(F64) if c["cap"] else None,
                live=live, dead=dead, dirty=dirty, clean=~dead & ~dirty)


def groups(rf):
    return [(n, rf[n]) for n in ("clean", "dirty") if bool(rf[n].any())]


def bounds(c, rf):
    """-> {(dtype name, group): (rel-L2 bound, worst-row bound)} from the references alone - the rules of test_gemma_gpu.test_flash_attn_softcap:
    bf16 max(1.5 x the rounding-point variant's error, 2^-9); fp32 1e-5 / 1e-4, or 4 x the float32 host evaluation's error with a cap"""
    out = {}
    for name, rows in groups(rf):
        t, va = rf["truth"][rows], rf["variant"][rows]
        out["bf16", name] = (max(1.5 * _rel_l2(va, t), FLOOR), max(1.5 * worst_row(va, t), FLOOR))
        if c["cap"]:
            h = rf["host32"][rows]
            out["f32", name] = (max(1e-5, 4 * _rel_l2(h, t)), max(1e-4, 4 * worst_row(h, t)))
        else:
            out["f32", name] = (1e-5, 1e-4)
    return out


def judge(c, rf, got, bf16: bool):
    """-> (worst error / bound over the groups and the two metrics, lines). got [B, L, H, 256]; a NaN anywhere is an infinite ratio. The dead rows are
    in no group: the caller asserts them to be exactly zero."""
    bd, worst, lines = bounds(c, rf), 0.0, []
    dt = "bf16" if bf16 else "f32"
    for name, rows in groups(rf):
        g, t = got[rows].to(F64), rf["truth"][rows]
        e, ew = _rel_l2(g, t), worst_row(g, t)
        b, bw = bd[dt, name]
        ratio = max(e / b, ew / bw)
        worst = max(worst, ratio if ratio == ratio else float("inf"))
        lines.append(f"{c['id']} {dt} {name} ({int(rows.sum())} rows): rel_l2 {e:.3e} (bound {b:.3e}) worst row {ew:.3e} (bound {bw:.3e})")
    return worst, lines
