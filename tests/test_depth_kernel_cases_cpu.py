"""What the case table of the depth-kernel sweep (tests/depth_kernel_cases.py) promises, checked on the host: every case lands on the vector or scalar
path and in the branch its name says and the table holds every size the sweep is about; the rounding-point variants of depth_ref sit within 4x
torch's own fp32 distance of F.interpolate in float64; the device-side judgement passes the correct reference rounded as each entry rounds, on every
case, and fails every slip on at least one; and depth_ref.resize_pil_tables is PIL's BICUBIC on the sizes the device test resizes. No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import depth_kernel_cases as K
from tests import depth_ref as R
from tests import image_ref
from tests.test_image_ref_cpu import RESIZE_PAIRS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BICUBIC_PAIRS = RESIZE_PAIRS + [((480, 640), (392, 518)), ((45, 33), (70, 56))]          # the second two: the processor's own ratios


def _by(kernel, **kv):
    return [c for c in K.cases(kernel) if all(c[k] == v for k, v in kv.items())]


# ---- the table is what it claims ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", K.KERNELS)
def test_every_case_takes_the_path_it_names(kernel):
    for c in K.cases(kernel):
        for dt in K.dtypes(kernel):
            assert K.VEC[kernel](c, K.ESIZE[dt]) == (c["path"] == "vec"), (kernel, c["id"], dt)
        assert ("+" in c["id"].replace("kp+64", "").replace("ld+8", "")) <= (c["path"] == "scalar"), c["id"]      # a case named after an offset is a scalar one
    if kernel != "bicubic":
        assert {c["path"] for c in K.cases(kernel)} == {"vec", "scalar"}, kernel


def test_the_named_branches_are_entered():
    # u8_to_patches: the column loop's second trip needs Kp > 128 lanes x 8 columns, with image data behind column 1024
    for P, trips in ((19, 2), (64, 12)):
        for c in _by("patches", P=P):
            assert -(-c["Kp"] // 1024) >= trips and 3 * P * P > 1024, c["id"]
    assert all(c["Kp"] <= 1024 for c in K.cases("patches") if c["P"] <= 16)
    assert _by("patches", P=19, path="scalar") and _by("patches", P=14, path="scalar") and _by("patches", margin=(0, 0))
    assert any(c["ld"] >= c["Kp"] + 8 and c["path"] == "vec" for c in K.cases("patches")) and any(c["ld"] == c["Kp"] for c in K.cases("patches")) and any(c["Kp"] > (3 * c["P"] ** 2 + 63) // 64 * 64 for c in K.cases("patches"))
    # deconv: ragged channels are scalar by the host's rule; pad groups (c0 >= Cout) run under vec = 1; each way into the scalar path on whole channels
    ragged = [c for c in K.cases("deconv") if c["Cout"] % 8]
    assert {c["Cout"] for c in ragged} == {1, 20} and all(c["path"] == "scalar" for c in ragged)
    assert any(c["path"] == "vec" and c["Cp"] >= c["Cout"] + 8 for c in K.cases("deconv"))
    whole = [c for c in K.cases("deconv") if c["Cout"] % 8 == 0 and c["path"] == "scalar"]
    assert any(c["ld"] % 4 for c in whole) and any(c["bias_off"] for c in whole) and any(c["out_off"] for c in whole)
    assert any(c["ld"] > c["f"] ** 2 * c["Cout"] and c["path"] == "vec" for c in K.cases("deconv"))
    # head_out: the ragged last group under both paths, a row that is no multiple of 16 bytes in either type, misaligned x and w
    head = K.cases("head")
    assert any(c["C"] % 8 and c["path"] == "vec" for c in head) and any(c["C"] % 8 and c["path"] == "scalar" for c in head)
    assert any((c["Cp"] * 2) % 16 and (c["Cp"] * 4) % 16 for c in head) and any(c["x_off"] for c in head) and any(c["w_off"] for c in head)
    assert any(c["C"] > 32 for c in head)                                                 # a lane's second step (c0 += 32)
    for c in head:
        if c["id"].endswith("-pm100"):
            v = K.refs("head", c["id"])["v"]
            assert float(v.min()) <= -100 and float(v.max()) >= 100, (c["id"], float(v.min()), float(v.max()))
    # minmax: both strided rounds and the ragged tail hold an extreme in some case, as minimum and as maximum
    for H, W in ((300, 500), (257, 523), (1, 1023), (1, 1025)):
        HW, placed = H * W, _by("minmax", H=H, W=W, kind="placed", d_off=0, out_off=0)
        want = set(K.mm_indices(HW))
        assert {c["lo"] for c in placed} == want and {c["hi"] for c in placed} == want, (H, W)
        assert {c["ch"] for c in placed} == {1, 3}
        if HW > K.MM_ROUND:
            assert {K.MM_ROUND - 1, K.MM_ROUND, 2 * K.MM_ROUND - 1, HW - 1, 0, HW - (HW % 4 or 4)} == want
    assert (257 * 523) % 4 and 257 * 523 > 2 * K.MM_ROUND and 1023 % 4 and 1025 % 4
    assert any(c["d_off"] and c["HW"] % 4 == 0 and not c["out_off"] for c in K.cases("minmax")) and any(c["out_off"] % 4 and not c["d_off"] for c in K.cases("minmax"))
    for kind in ("subnormal", "offset"):
        for c in _by("minmax", kind=kind):
            d = K.data("minmax", c["id"])["d"].double()
            spread = d.max(1).values - d.min(1).values
            assert bool(torch.isfinite(d).all()) and bool((spread > 0).all())
            assert bool((spread < 2.0 ** -126).all()) if kind == "subnormal" else bool((spread <= 2.1e24).all() and (d.min() > 9e29))
    for c in _by("minmax", kind="placed"):
        d = K.data("minmax", c["id"])["d"]
        assert len(d.unique()) == 3 and int((d[0] == d[0].min()).sum()) == 1 and int(d[0].argmin()) == c["lo"] and int(d[1].argmax()) == c["lo"]


def test_the_table_holds_the_sizes_the_sweep_is_about():
    bl = K.cases("bilinear")
    shapes = {(c["B"], c["src"], c["dst"], c["C"]) for c in bl}
    assert {(1, (37, 37), (74, 74), 8), (1, (37, 37), (74, 74), 64), (1, (148, 148), (296, 296), 8), (1, (296, 296), (518, 518), 8), (2, (74, 37), (148, 74), 8)} <= shapes
    for src, dst in (((37, 37), (74, 74)), ((148, 148), (296, 296)), ((296, 296), (518, 518)), ((74, 37), (148, 74)), ((5, 7), (5, 7)), ((100, 60), (37, 23))):
        assert {c["align"] for c in bl if c["src"] == src and c["dst"] == dst and c["C"] == 8} == {True, False}
    assert {c["C"] for c in bl} >= {8, 24, 64, 200} and any(c["B"] == 3 for c in bl)
    assert any(c["src"][0] == 1 for c in bl) and any(c["src"][1] == 1 for c in bl) and any(c["dst"][0] == 1 for c in bl) and any(c["dst"][1] == 1 for c in bl)
    assert any((c["B"] * c["dst"][0] * c["dst"][1] * c["C"] // 8) % 256 and c["B"] * c["dst"][0] * c["dst"][1] * c["C"] // 8 > 256 for c in bl)
    bc = {(c["src"], c["dst"]) for c in K.cases("bicubic")}
    assert {((518, 518), (1080, 1920)), ((518, 518), (519, 517)), ((518, 518), (224, 224)), ((1, 1), (7, 300))} <= bc
    assert {d[1] for _, d in bc} >= {255, 256, 257, 1} and any(c["B"] == 3 for c in K.cases("bicubic"))
    assert {s[0] for s, _ in bc} >= {2, 3} and {s[1] for s, _ in bc} >= {2, 3}
    dc = K.cases("deconv")
    assert {c["f"] for c in dc} == {1, 2, 4, 16} and {(c["Cout"], c["Cp"]) for c in dc} == {(1, 8), (20, 24), (24, 64), (48, 64), (96, 128), (384, 384)}
    assert {(c["h"], c["w"]) for c in _by("deconv", f=2, Cout=96)} >= {(1, 1), (3, 5), (37, 37)}
    hd = K.cases("head")
    assert {c["C"] for c in hd} == {1, 7, 32, 33, 100} and {c["npix"] for c in hd} == {1, 63, 65, 257, 518 * 518}
    for key in ("C", "npix"):
        for v in {c[key] for c in hd}:
            assert {c["metric"] for c in hd if c[key] == v} == {True, False}
    pt = K.cases("patches")
    assert {c["P"] for c in pt} == {1, 14, 16, 19, 64} and all({c["C"] for c in _by("patches", P=P)} == {1, 3} for P in (1, 14, 16, 19, 64))
    assert {c["n"] for c in K.cases("relu")} == {8, 4104}
    x = K.data("relu", "n8")["x"]
    assert bool(x.isnan().any()) and bool(((x == 0) & torch.signbit(x)).any()) and bool(((x == 0) & ~torch.signbit(x)).any())


# ---- the variants against float64 ----------------------------------------------------------------------------------------------------------------
INTERP = [("bilinear", i) for i in K.case_ids("bilinear")] + [("bicubic", i) for i in K.case_ids("bicubic")]


@pytest.mark.parametrize("kernel,cid", INTERP, ids=[f"{k}-{i}" for k, i in INTERP])
def test_variant_is_as_close_to_float64_as_torch_fp32(kernel, cid):
    """max-abs and rel-L2 of the variant (weights in float32, taps in float64) against F.interpolate in float64: at most 4x those of torch's own fp32
    run on the case. The yardstick has the floor the live c has (one 2^-24 of the inputs' magnitude): on a copy torch's error is exactly 0."""
    rf = K.refs(kernel, cid)
    ev, et = (rf["variant"] - rf["truth"]).abs().max(), (rf["t32"].double() - rf["truth"]).abs().max()
    rv, rt = R.rel_l2(rf["variant"], rf["truth"]), R.rel_l2(rf["t32"], rf["truth"])
    print(f"[depth-cases] {kernel} {cid}: variant {float(ev):.3e} / {rv:.3e}, torch fp32 {float(et):.3e} / {rt:.3e} (c {rf['c']:.1f})")
    assert float(ev) <= K.MARGIN * max(float(et), K.U * rf["scale"]), (cid, float(ev), float(et))
    assert rv <= K.MARGIN * max(rt, K.U), (cid, rv, rt)


# ---- the judgement passes what is right and fails what is wrong ----------------------------------------------------------------------------------------
ALL = [(k, i) for k in K.KERNELS for i in K.case_ids(k)]


@pytest.mark.parametrize("kernel,cid", ALL, ids=[f"{k}-{i}" for k, i in ALL])
def test_the_correct_reference_stays_inside_its_bound(kernel, cid):
    for dt in K.dtypes(kernel):
        ratio, line = K.judge(kernel, cid, dt, K.correct(kernel, cid, dt))
        assert ratio <= 1.0, line


def _size(kernel, c):
    return {"bilinear": lambda: c["B"] * c["dst"][0] * c["dst"][1] * c["C"], "bicubic": lambda: c["B"] * c["dst"][0] * c["dst"][1], "head": lambda: c["npix"] * c["Cp"],
            "deconv": lambda: c["B"] * c["h"] * c["w"] * c["f"] ** 2 * c["Cp"], "minmax": lambda: c["HW"], "patches": lambda: c["H"] * c["W"]}[kernel]()


@pytest.mark.parametrize("slip", list(K.SLIPS))
def test_every_slip_is_caught(slip):
    kernel, wrong = K.SLIPS[slip]
    caught = []
    for c in sorted(K.cases(kernel), key=lambda c: _size(kernel, c)):
        for dt in K.dtypes(kernel):
            got = wrong(c, K.data(kernel, c["id"]), dt)
            if K.judge(kernel, c["id"], dt, got)[0] > 1.0:
                caught.append((c["id"], dt))
        if len(caught) >= 2 or (caught and _size(kernel, c) > 100000):
            break
    print(f"[depth-cases] {slip}: caught by {caught}")
    assert caught, slip


# ---- BICUBIC resize: the reference of the device test is PIL's ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", BICUBIC_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_resize_pil_tables_bicubic_is_pils(pair):
    Image = pytest.importorskip("PIL.Image")
    (H, W), (h, w) = pair
    img = image_ref.synth(1, H, W, 3, seed=47)[0]
    assert np.array_equal(R.resize_pil_tables(img, h, w), np.array(Image.fromarray(img).resize((w, h), Image.BICUBIC)))
    gray = img[..., :1]
    assert np.array_equal(R.resize_pil_tables(gray, h, w)[..., 0], np.array(Image.fromarray(gray[..., 0], mode="L").resize((w, h), Image.BICUBIC)))


def test_resize_pil_tables_bicubic_large_ratio_is_pils():
    Image = pytest.importorskip("PIL.Image")
    img = image_ref.synth(1, 16, 20000, 3, seed=9)[0]
    assert np.array_equal(R.resize_pil_tables(img, 16, 300), np.array(Image.fromarray(img).resize((300, 16), Image.BICUBIC)))


def test_the_header_states_relus_nan_contract():
    with open(os.path.join(ROOT, "include", "unigen_hip.h")) as f:
        text = f.read()
    comment = text[:text.index("int ug_relu(")].rsplit("/*", 1)[1]
    assert "NaN propagates" in comment and "-0 stays -0" in comment
