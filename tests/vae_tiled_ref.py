"""References for AutoencoderKL tiling (diffusers 0.32.2 `tiled_decode` / `tiled_encode`, restated: the source is not part of this repository, so
parity with it is unpinned, as for the rest of the VAE). Plain torch, any device; tests/test_vae_tiled_ref_cpu.py pins the two forms to each other.

LITERAL  `tiled_literal`: diffusers' algorithm step by step - nested loops over tile starts, every tile through the per-tile callable, then in
         row-major order blend_v with the (already blended) upper tile, blend_h with the (already blended) left tile, both in place, the
         [:crop, :crop] corner of each tile, torch.cat along W, torch.cat along H.
CLOSED   `closed_form_tile`: one tile's canvas region from the four RAW tiles (itself, upper, left, upper-left), the form ug_vae_tile_blend
         evaluates (include/unigen_hip.h). Valid while a full tile has at least 2 E rows / columns (tile_overlap_factor <= 0.5).

Rounding points, the same in both: `a * (1 - k / e) + b * (k / e)` on tensors of dtype T is three tensor ops - the two weights are Python doubles
cast to fp32 (torch's GPU kernels multiply a tensor by a Python scalar in fp32; its CPU bf16 kernels round the scalar to bf16 first, which is NOT
what is restated here, so `_lerp` spells the casts out and gives the same bits on every device), each product is rounded to T, and so is the sum.
"""
import torch

F32 = torch.float32


def _lerp(a, b, k, e, slip=None):
    """rnd(rnd(a * f32(1 - k / e)) + rnd(b * f32(k / e))), rnd = round to the tensors' dtype."""
    dt = a.dtype
    wa, wb = 1 - k / e, k / e                      # Python doubles
    if slip == "weights_swapped":
        wa, wb = wb, wa
    wa, wb = torch.tensor(wa, dtype=F32, device=a.device), torch.tensor(wb, dtype=F32, device=a.device)
    pa, pb = a.to(F32) * wa, b.to(F32) * wb
    if slip != "drop_rounding":
        pa, pb = pa.to(dt), pb.to(dt)
    return (pa.to(F32) + pb.to(F32)).to(dt)


def blend_v(a, b, extent):
    e = min(a.shape[2], b.shape[2], extent)
    for y in range(e):
        b[:, :, y, :] = _lerp(a[:, :, -e + y, :], b[:, :, y, :], y, e)
    return b


def blend_h(a, b, extent):
    e = min(a.shape[3], b.shape[3], extent)
    for x in range(e):
        b[:, :, :, x] = _lerp(a[:, :, :, -e + x], b[:, :, :, x], x, e)
    return b


def make_tiles(x, fn, tile, stride):
    """rows[i][j] = fn(x[:, :, i:i+tile, j:j+tile]) over range(0, H, stride) x range(0, W, stride) (the last row / column of tiles is smaller)."""
    rows = []
    for i in range(0, x.shape[2], stride):
        row = []
        for j in range(0, x.shape[3], stride):
            row.append(fn(x[:, :, i:i + tile, j:j + tile]))
        rows.append(row)
    return rows


def literal_from_tiles(rows, extent, crop):
    """The blend / crop / cat half of diffusers' tiled_decode on raw tiles (cloned: the blends are in place)."""
    rows = [[t.clone() for t in row] for row in rows]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, extent)
            if j > 0:
                tile = blend_h(row[j - 1], tile, extent)
            result_row.append(tile[:, :, :crop, :crop])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


def tiled_literal(x, fn, tile, stride, extent, crop):
    return literal_from_tiles(make_tiles(x, fn, tile, stride), extent, crop)


def closed_form_tile(T, U, Lf, UL, extent, crop, slip=None):
    """Canvas region of tile T from the RAW tiles: out(y, x) for y < min(T.H, crop), x < min(T.W, crop), element by element as the header states it.
    slip: one of the mistakes test_vae_tiled_ref_cpu.py shows to be visible - 'h_before_v', 'raw_upper', 'weights_swapped', 'drop_rounding'."""
    h, w = min(T.shape[2], crop), min(T.shape[3], crop)
    ev = min(U.shape[2], T.shape[2], extent) if U is not None else 0
    eh = min(Lf.shape[3], T.shape[3], extent) if Lf is not None else 0
    lerp = lambda a, b, k, e: _lerp(a, b, k, e, slip if slip in ("weights_swapped", "drop_rounding") else None)
    out = torch.empty(T.shape[0], T.shape[1], h, w, dtype=T.dtype, device=T.device)

    def upper(y, x):        # U'(U.H - ev + y, x): the upper tile after ITS blend_h with the upper-left tile
        r = U.shape[2] - ev + y
        if x < eh and slip != "raw_upper":
            return lerp(UL[:, :, r, UL.shape[3] - eh + x], U[:, :, r, x], x, eh)
        return U[:, :, r, x]

    def left(y, x):         # Lf'(y, Lf.W - eh + x): the left tile after ITS blend_v with the upper-left tile
        c = Lf.shape[3] - eh + x
        if y < ev:
            return lerp(UL[:, :, UL.shape[2] - ev + y, c], Lf[:, :, y, c], y, ev)
        return Lf[:, :, y, c]

    for y in range(h):
        for x in range(w):
            t = T[:, :, y, x]
            if slip == "h_before_v":
                if x < eh:
                    t = lerp(left(y, x), t, x, eh)
                if y < ev:
                    t = lerp(upper(y, x), t, y, ev)
            else:
                if y < ev:
                    t = lerp(upper(y, x), t, y, ev)
                if x < eh:
                    t = lerp(left(y, x), t, x, eh)
            out[:, :, y, x] = t
    return out


def closed_form_from_tiles(rows, extent, crop, slip=None):
    out_rows = []
    for i, row in enumerate(rows):
        out_rows.append(torch.cat([closed_form_tile(t, rows[i - 1][j] if i else None, row[j - 1] if j else None, rows[i - 1][j - 1] if i and j else None,
                                                    extent, crop, slip) for j, t in enumerate(row)], dim=3))
    return torch.cat(out_rows, dim=2)


def plan(tile_in, scale, f, down=False):
    """diffusers' sizes for a tile of `tile_in` on the input side of a decoder that grows sizes by `scale` (down: an encoder that shrinks them):
    -> (stride on the input side, blend extent and crop on the output side)."""
    tile_out = tile_in // scale if down else tile_in * scale
    extent = int(tile_out * f)
    return int(tile_in * (1 - f)), extent, tile_out - extent


# Canvas shapes on the input side for a tile of 8 and a decoder scale of 2 (output tile 16): with f = 0.25 the stride is 6, E = 4, crop 12.
#   20: tiles 8, 8, 8, 2 (several full tiles; the last one is exactly E wide on the output side)      19: last tile 1 -> 2 < E
#   21: last tile 3 -> 6, between E and 2 E         6: one row / column of tiles (range(0, n, stride) starts a second tile as soon as n > stride:
#   a canvas of 7 or 8 rows is ONE tile high for the routing and still two tiles high here, 7 + 1 or 8 + 2 rows)
# with f = 0.5: stride 4, E = 8, crop 8 (a full tile is exactly 2 E); with f = 0: stride 8, E = 0, crop 16 (plain tiling).
TILE, SCALE = 8, 2
CASES = [dict(B=1, H=20, W=20, f=0.25), dict(B=2, H=19, W=21, f=0.25), dict(B=1, H=21, W=19, f=0.25), dict(B=1, H=6, W=20, f=0.25),
         dict(B=2, H=21, W=6, f=0.25), dict(B=1, H=14, W=19, f=0.5), dict(B=2, H=13, W=4, f=0.5), dict(B=1, H=19, W=17, f=0.0),
         dict(B=1, H=7, W=15, f=0.25)]


def random_tiles(case, C, dtype, seed=0, scale=SCALE, tile=TILE):
    """Raw tiles of a case: independent N(0, 1) values (a decoder's output is whatever it is: the blend must hold for any), -> (rows, extent, crop)."""
    g = torch.Generator().manual_seed(seed)
    stride, extent, crop = plan(tile, scale, case["f"])
    x = torch.zeros(case["B"], 1, case["H"], case["W"])
    fn = lambda t: torch.randn(t.shape[0], C, t.shape[2] * scale, t.shape[3] * scale, generator=g).to(dtype)
    return make_tiles(x, fn, tile, stride), extent, crop
