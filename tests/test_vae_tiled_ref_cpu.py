"""AutoencoderKL tiling without a GPU: the literal restatement of diffusers' tiled_decode / tiled_encode against the four-tile closed form that
ug_vae_tile_blend evaluates (tests/vae_tiled_ref.py) - bit for bit, bf16 and fp32 - every plausible slip of the closed form shown to fail that
comparison, and the host logic of unigen_amd/vae.py and the pipelines: derived sizes, routing thresholds, refusals, forwarders."""
import importlib

import pytest
import torch

from tests import vae_tiled_ref as TR

BF, F32 = torch.bfloat16, torch.float32
TINY = dict(block_out_channels=(64, 128), layers_per_block=1, norm_num_groups=32)
SLIPS = ["h_before_v", "raw_upper", "weights_swapped", "drop_rounding"]


def _id(c):
    return f"B{c['B']}_{c['H']}x{c['W']}_f{c['f']}"


def test_case_table_covers_what_it_claims():
    """several full tiles each way; a last tile narrower than E; one between E and 2 E; a single row and a single column of tiles; f in {0, 0.25, 0.5}; B = 2"""
    seen = set()
    for c in TR.CASES:
        stride, E, crop = TR.plan(TR.TILE, TR.SCALE, c["f"])
        seen.add(("f", c["f"]))
        seen.add(("B", c["B"]))
        for n, other in ((c["H"], c["W"]), (c["W"], c["H"])):
            sizes = [min(TR.TILE, n - i) * TR.SCALE for i in range(0, n, stride)]
            if len(sizes) == 1 and other > TR.TILE:
                seen.add(("single", n == c["H"]))
            if sum(s == TR.TILE * TR.SCALE for s in sizes) >= 3:
                seen.add("several full")
            if E and len(sizes) > 1 and sizes[-1] < E:
                seen.add("last < E")
            if E and len(sizes) > 1 and E < sizes[-1] < 2 * E:
                seen.add("E < last < 2E")
    assert {("f", 0.0), ("f", 0.25), ("f", 0.5), ("B", 2), ("single", True), ("single", False), "several full", "last < E", "E < last < 2E"} <= seen, seen


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", TR.CASES, ids=_id)
def test_literal_equals_closed_form_bit_for_bit(case, dt):
    rows, E, crop = TR.random_tiles(case, 3, dt, seed=1)
    lit, closed = TR.literal_from_tiles(rows, E, crop), TR.closed_form_from_tiles(rows, E, crop)
    assert lit.shape == (case["B"], 3, case["H"] * TR.SCALE, case["W"] * TR.SCALE)          # output = input x scale factor
    assert lit.dtype == dt and torch.equal(lit, closed)
    assert all(torch.isfinite(t.float()).all() for row in rows for t in row)                  # the inputs were not modified into nonsense


def test_tiled_literal_runs_the_callable_per_tile_and_mirrors_for_encode():
    """the driver: tile starts, smaller last tiles, the callable's own scale; an encoder (sizes shrink) gives input / scale"""
    calls = []

    def dec(t):
        calls.append(tuple(t.shape))
        return t.repeat_interleave(2, 2).repeat_interleave(2, 3) + len(calls)
    x = torch.arange(2 * 1 * 19 * 6, dtype=F32).view(2, 1, 19, 6)
    stride, E, crop = TR.plan(8, 2, 0.25)
    out = TR.tiled_literal(x, dec, 8, stride, E, crop)
    assert out.shape == (2, 1, 38, 12) and calls == [(2, 1, 8, 6), (2, 1, 8, 6), (2, 1, 7, 6), (2, 1, 1, 6)]
    stride, E, crop = TR.plan(16, 2, 0.25, down=True)
    assert (stride, E, crop) == (12, 2, 6)
    enc = lambda t: t[:, :, ::2, ::2].clone()
    x = torch.randn(1, 2, 40, 28, generator=torch.Generator().manual_seed(0))
    assert TR.tiled_literal(x, enc, 16, stride, E, crop).shape == (1, 2, 20, 14)
    # a constant image through an identity-like tile function stays constant: the two weights sum to one
    one = torch.full((1, 1, 20, 20), 3.0)
    assert torch.equal(TR.tiled_literal(one, lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3), 8, *TR.plan(8, 2, 0.25)), torch.full((1, 1, 40, 40), 3.0))


@pytest.mark.parametrize("slip", SLIPS)
def test_every_slip_of_the_closed_form_fails(slip):
    """a closed form with one plausible mistake differs from the literal algorithm somewhere on the case table, in both dtypes - so exact equality
    with the literal reference (which is what the GPU test asks of the kernel) cannot be met by a kernel that makes it. A dropped rounding of a
    product is no mistake in fp32, where the product already is the tensor's type: bf16 alone can see it."""
    for dt in (BF,) if slip == "drop_rounding" else (BF, F32):
        bad = 0
        for case in TR.CASES:
            rows, E, crop = TR.random_tiles(case, 3, dt, seed=2)
            bad += int(not torch.equal(TR.literal_from_tiles(rows, E, crop), TR.closed_form_from_tiles(rows, E, crop, slip)))
        assert bad >= 1, (slip, dt)


def test_slips_touch_only_what_they_should():
    """h_before_v and raw_upper live in the corner where both blends meet: a single row of tiles cannot see them, a 2 x 2 grid does"""
    row_only = next(c for c in TR.CASES if c["H"] <= TR.plan(TR.TILE, TR.SCALE, 0.25)[0] and c["f"] == 0.25)
    rows, E, crop = TR.random_tiles(row_only, 3, F32, seed=3)
    for slip in ("h_before_v", "raw_upper"):
        assert torch.equal(TR.literal_from_tiles(rows, E, crop), TR.closed_form_from_tiles(rows, E, crop, slip))
    rows, E, crop = TR.random_tiles(dict(B=1, H=12, W=12, f=0.25), 3, F32, seed=3)
    lit = TR.literal_from_tiles(rows, E, crop)
    for slip in ("h_before_v", "raw_upper"):
        d = (lit != TR.closed_form_from_tiles(rows, E, crop, slip))[0, 0]
        assert d.any() and not d[:12].any() and not d[:, :12].any() and not d[12 + E:].any() and not d[:, 12 + E:].any()      # the corner of tile (1, 1) only


# ----------------------------------------------------------------------------------------------------------------------------------
# host logic (no launches: every refusal below happens before the first kernel)
# ----------------------------------------------------------------------------------------------------------------------------------
def _vae(**kw):
    return importlib.import_module("unigen_amd.vae").AutoencoderKL.from_config(dict(kw), device="cpu")


def test_default_sizes_and_switches():
    cls = importlib.import_module("unigen_amd.vae").AutoencoderKL
    flux = cls.from_config({}, device="meta")
    assert (flux.tile_sample_min_size, flux.tile_latent_min_size, flux.tile_overlap_factor) == (1024, 128, 0.25)
    assert flux.use_tiling is False and flux.use_slicing is False
    v = _vae(sample_size=64, **TINY)
    assert (v.tile_sample_min_size, v.tile_latent_min_size) == (64, 32)
    v.enable_tiling(); assert v.use_tiling is True
    v.enable_tiling(False); assert v.use_tiling is False
    v.enable_tiling(); v.disable_tiling(); assert v.use_tiling is False
    v.enable_slicing(); assert v.use_slicing is True
    v.disable_slicing(); assert v.use_slicing is False
    v.tile_latent_min_size, v.tile_sample_min_size, v.tile_overlap_factor = 16, 32, 0.5          # plain settable attributes
    assert (v.tile_latent_min_size, v.tile_sample_min_size, v.tile_overlap_factor) == (16, 32, 0.5)
    assert callable(v.tiled_encode) and callable(v.tiled_decode)


def test_routing_thresholds(monkeypatch):
    """tiled only with use_tiling and H or W ABOVE the tile size of that side; an input exactly at tile size stays on the untiled code;
    slicing sends every sample through the same route"""
    v = _vae(**TINY)
    v.tile_latent_min_size, v.tile_sample_min_size = 16, 32
    seen = []
    monkeypatch.setattr(v, "_decode", lambda z, d, a: seen.append(("plain", tuple(z.shape))) or torch.zeros(z.shape[0], 3, 1, 1))
    monkeypatch.setattr(v, "_tiled_decode", lambda z, d, a: seen.append(("tiled", tuple(z.shape))) or torch.zeros(z.shape[0], 3, 1, 1))
    monkeypatch.setattr(v, "_encode_moments", lambda x: seen.append(("plain", tuple(x.shape))) or (torch.zeros(x.shape[0], 32), x.shape[0], 1, 1))
    monkeypatch.setattr(v, "_tiled_moments", lambda x: seen.append(("tiled", tuple(x.shape))) or (torch.zeros(x.shape[0], 32), x.shape[0], 1, 1))
    z, big_h, big_w = torch.zeros(1, 16, 16, 16), torch.zeros(1, 16, 17, 16), torch.zeros(1, 16, 8, 24)
    for t in (z, big_h, big_w):
        v.decode(t)
    v.enable_tiling()
    for t in (z, big_h, big_w):
        v.decode(t)
    v.decode_scaled(big_w)
    assert [s[0] for s in seen] == ["plain"] * 3 + ["plain", "tiled", "tiled", "tiled"]
    seen.clear()
    x, xb = torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 40)
    v.encode(x); v.encode(xb)
    v.disable_tiling(); v.encode(xb)
    assert [s[0] for s in seen] == ["plain", "tiled", "plain"]
    seen.clear()
    v.enable_slicing(); v.enable_tiling()
    out = v.decode(torch.zeros(3, 16, 17, 16)).sample
    assert seen == [("tiled", (1, 16, 17, 16))] * 3 and out.shape[0] == 3
    seen.clear()
    d = v.encode(torch.zeros(3, 3, 32, 32)).latent_dist
    assert seen == [("plain", (1, 3, 32, 32))] * 3 and d._m.shape == (3, 32) and d._shape[0] == 3
    seen.clear()
    v.decode(torch.zeros(1, 16, 17, 16))                    # B = 1: slicing changes nothing
    assert seen == [("tiled", (1, 16, 17, 16))]


def test_overlap_factor_outside_the_closed_form_is_refused():
    v = _vae(**TINY)
    v.tile_latent_min_size, v.tile_sample_min_size = 16, 32
    for f in (0.51, 0.75, -0.1, 1.0):
        v.tile_overlap_factor = f
        with pytest.raises(ValueError, match=r"tile_overlap_factor must be within \[0, 0.5\].*one pass"):
            v.tiled_decode(torch.zeros(1, 16, 32, 32))
        with pytest.raises(ValueError, match="tile_overlap_factor"):
            v.tiled_encode(torch.zeros(1, 3, 64, 64))
    # sizes that do not fit each other (the default sample-side size left in place next to a small latent tile) are refused too, by name
    v.tile_overlap_factor, v.tile_sample_min_size = 0.25, 1024
    with pytest.raises(ValueError, match="do not fit each other"):
        v.tiled_decode(torch.zeros(1, 16, 32, 32))


def test_tile_shapes_are_checked_before_any_launch():
    """the mid-block attention's H*W % 64 rule holds per tile; a canvas whose LAST tile breaks it is refused with the untiled path's words before the
    first tile runs (on this machine a launch would fail differently: there is no device)"""
    L = importlib.import_module("unigen_amd.lib")
    v = _vae(**TINY)
    v.tile_latent_min_size, v.tile_sample_min_size = 16, 32
    with pytest.raises(L.UniGenHipError, match=r"mid-block attention needs H\*W at the latent resolution to be a multiple of 64 \(got 80\)"):
        v.tiled_decode(torch.zeros(1, 16, 32, 29))          # tiles of 16, 16, 5 columns: 16 x 5 = 80
    with pytest.raises(L.UniGenHipError, match=r"multiple of 64 \(got 112\)"):
        v.tiled_encode(torch.zeros(1, 3, 32, 62))           # sample tiles 32, 32, 14 wide -> latent 16 x 7
    with pytest.raises(ValueError, match="multiples of 2"):
        v.tiled_encode(torch.zeros(1, 3, 64, 63))
    v2 = _vae(mid_block_add_attention=False, **TINY)      # no attention, no rule: the plan itself passes
    v2.tile_latent_min_size, v2.tile_sample_min_size = 16, 32
    assert v2._tile_plan(32, 29, 16, 32, down=False) == (12, 8, 24, 2)
    assert v2._tile_plan(64, 54, 32, 16, down=True) == (24, 4, 12, 2)


@pytest.mark.parametrize("mod,name", [("src.UniGenPipeline", "UniGenFLUXPipeline"), ("src.UniGenPipeline", "UniGenSD3Pipeline"), ("unigen_amd.pipeline", "UniGenFLUXPipeline")])
def test_pipeline_forwarders(mod, name):
    cls = getattr(importlib.import_module(mod), name)
    pipe = cls.from_pretrained(None, transformer=None)
    for fn in ("enable_vae_tiling", "disable_vae_tiling", "enable_vae_slicing", "disable_vae_slicing"):
        with pytest.raises(RuntimeError, match=rf"{fn}\(\): no VAE is attached"):
            getattr(pipe, fn)()
    pipe.vae = v = _vae(**TINY)
    pipe.enable_vae_tiling(); assert v.use_tiling and not v.use_slicing
    pipe.enable_vae_slicing(); assert v.use_tiling and v.use_slicing
    pipe.disable_vae_tiling(); assert not v.use_tiling and v.use_slicing
    pipe.disable_vae_slicing(); assert not v.use_tiling and not v.use_slicing


def test_blend_abi_layout_and_refusals_before_any_launch(tmp_path):
    """the ctypes mirrors have the C layout of include/unigen_hip.h (checked against a compile of the header), and every malformed descriptor is
    turned away with its own code and words before a kernel is launched - so this runs without a device"""
    import ctypes
    import os
    import subprocess
    lib = importlib.import_module("unigen_amd.lib")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include "unigen_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu", sizeof(ug_vae_tile), offsetof(ug_vae_tile, sx), '
           'sizeof(ug_vae_blend_desc), offsetof(ug_vae_blend_desc, UL), offsetof(ug_vae_blend_desc, out), offsetof(ug_vae_blend_desc, E));return 0;}')
    exe = str(tmp_path / "ug_blend_layout")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(root, "include"), "-o", exe], input=src.encode(), check=True)
    sizes = list(map(int, subprocess.run([exe], capture_output=True, check=True).stdout.split()))
    T, D = lib.VaeTile, lib.VaeBlendDesc
    assert sizes == [ctypes.sizeof(T), T.sx.offset, ctypes.sizeof(D), D.UL.offset, D.out.offset, D.E.offset]
    assert lib.SIGNATURES["ug_vae_tile_blend_f32"] == lib.SIGNATURES["ug_vae_tile_blend"] and lib._F32_TWINS["ug_vae_tile_blend_f32"] == "ug_vae_tile_blend"
    cdll = lib.load()
    assert cdll.ug_version() >= 230

    def tile(h, w, p=16):
        t = T()
        t.p, t.H, t.W, t.sb, t.sc, t.sy, t.sx = p, h, w, 3 * h * w, h * w, w, 1
        return t

    def desc(**kw):
        d = D()
        d.T, d.out, d.ob, d.oc, d.oy, d.ox, d.B, d.C, d.h, d.w, d.E = tile(8, 8), 16, 192, 64, 8, 1, 1, 3, 8, 8, 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for fn in (cdll.ug_vae_tile_blend, cdll.ug_vae_tile_blend_f32):
        assert fn(None, None) == lib.UG_ERR_BAD_SHAPE and b"null descriptor" in cdll.ug_last_error()
        assert fn(ctypes.byref(desc(B=0)), None) == lib.UG_OK                                   # nothing to do
        assert fn(ctypes.byref(desc(h=9)), None) == lib.UG_ERR_BAD_SHAPE                        # a crop larger than the tile
        assert fn(ctypes.byref(desc(out=None)), None) == lib.UG_ERR_BAD_SHAPE
        assert fn(ctypes.byref(desc(U=tile(8, 7))), None) == lib.UG_ERR_BAD_SHAPE and b"upper tile must have T's width" in cdll.ug_last_error()
        assert fn(ctypes.byref(desc(Lf=tile(7, 8))), None) == lib.UG_ERR_BAD_SHAPE
        assert fn(ctypes.byref(desc(U=tile(8, 8), Lf=tile(8, 8))), None) == lib.UG_ERR_BAD_SHAPE and b"upper-left tile" in cdll.ug_last_error()
        assert fn(ctypes.byref(desc(U=tile(8, 8), Lf=tile(8, 8), UL=tile(8, 7))), None) == lib.UG_ERR_BAD_SHAPE
        assert fn(ctypes.byref(desc(U=tile(8, 8), E=5)), None) == lib.UG_ERR_UNSUPPORTED and b"at least 2 E" in cdll.ug_last_error()
        assert fn(ctypes.byref(desc(Lf=tile(8, 9), E=5)), None) == lib.UG_ERR_UNSUPPORTED
        assert fn(ctypes.byref(desc(E=-1)), None) == lib.UG_ERR_BAD_SHAPE
