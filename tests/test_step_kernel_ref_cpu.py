"""The references of tests/step_kernel_ref.py against torch and the oracle, every committed case against the documented preconditions, the recorded
torch figures behind each bound, and the mutation checks: the plausible slips of each kernel, applied to the reference, must fail the very
judging function the GPU sweep (tests/test_fuzz_step_gpu.py) calls. No GPU."""
import math

import pytest
import torch

from oracle import unigen_ref as R
from tests import step_kernel_ref as SR

BF, F32, F64 = SR.BF, SR.F32, SR.F64
DTS = [BF, F32]


def _image(values, mask, dt):
    img = torch.full(mask.shape, SR.SENT, dtype=dt)
    img[mask] = values.reshape(-1).to(dt)
    return img


def _flat_mask(n, off=0):
    mask = torch.zeros(SR.GUARD + off + n + SR.GUARD, dtype=torch.bool)
    mask[SR.GUARD + off:SR.GUARD + off + n] = True
    return mask


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


# ----------------------------------------------------------------------------------------------------------------------------------
# pins
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_arithmetic_references_equal_torch(dt):
    """torch's CPU tensor ops round after every op in the tensor's dtype: the reference pipeline's expressions, evaluated by torch, bit for bit"""
    for c in SR.flat_cases("euler")[:6] + SR.flat_cases("euler")[7:]:
        x, v = SR.flat_data(c, dt)
        s0 = 0.9873806
        s1 = float(torch.tensor(s0, dtype=F32) + torch.tensor(c["dt"], dtype=F32))
        step = float(torch.tensor(s1, dtype=F32) - torch.tensor(s0, dtype=F32))            # the fp32 difference of fp32 sigmas, as the scheduler forms it
        assert torch.equal(SR.euler_step(x, v, step), R.euler_step(x, v, s0, s1)), c
    for c in SR.flat_cases("cfg")[:6] + SR.flat_cases("cfg")[7:]:
        u, t = SR.flat_data(c, dt)
        assert torch.equal(SR.cfg_combine(u, t, c["gs"]), u + c["gs"] * (t - u)), c            # src/UniGenPipeline.py:404-407
    g = torch.Generator().manual_seed(0)
    for rows, D, rp in [(7, 64, 3), (333, 200, 37), (12, 8, 12)]:
        a, b = SR.mags(g, (rows, D)).to(dt), SR.mags(g, (rows, D)).to(dt)
        assert torch.equal(SR.add(a, b), a + b)
        tab = SR.mags(g, (rp, D))
        idx = torch.arange(rows) % rp
        assert torch.equal(SR.add_rowbcast(a, tab, rp), (a.float() + tab[idx]).to(dt))            # PatchEmbed: (latent + pos_embed).to(latent.dtype)
        samples = (rows + rp - 1) // rp
        gate = SR.mags(g, (samples, D), -2, 1).to(dt)
        gexp = gate[torch.arange(rows) // rp]
        assert torch.equal(SR.gate_residual(b, a, gate, rp), b + gexp * a)            # x + gate.unsqueeze(1) * a
        assert torch.equal(SR.gate_residual(None, a, gate, rp), gexp * a)
        coef = 0.0123456
        assert torch.equal(SR.grad_scale(a, coef), (a.float() * torch.tensor(coef, dtype=F32)).to(dt))


def test_data_movement_references():
    g = torch.Generator().manual_seed(1)
    for B, Cc, H, W in SR.PACK_CASES[:1] + SR.PACK_CASES[2:6]:
        lat = torch.randn(B, Cc, H, W, generator=g)
        want = lat.view(B, Cc, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // 2) * (W // 2), Cc * 4)            # FluxPipeline._pack_latents
        assert torch.equal(SR.pack_latents(lat), want)
        back = want.view(B, H // 2, W // 2, Cc, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, H, W)            # _unpack_latents
        assert torch.equal(SR.unpack_latents(want, H, W), back) and torch.equal(back, lat)
    src = torch.randn(11, 64, generator=g)
    idx = torch.tensor([3, -1, 10, 0, 3, -2, 7], dtype=torch.int32)
    assert torch.equal(SR.gather_rows(src, idx), torch.where((idx >= 0)[:, None], src[idx.clamp_min(0).long()], torch.zeros(1, 64)))
    s = torch.randn(2, 5, 3, generator=g)
    t = SR.transpose(s, 8)
    assert torch.equal(t[:, :, :5], s.transpose(1, 2).contiguous()) and bool((t[:, :, 5:] == 0).all())


def test_timestep_gelu_linear_references():
    t = torch.tensor(SR.TS_T, dtype=F32)
    for dim in (2, 64, 256, 320, 1024):
        truth, a = SR.timestep_embed64(t, dim)
        assert torch.equal(SR.timestep_embed_torch32(t, dim), R.timestep_sinusoid(t, dim))
        assert float((truth - R.timestep_sinusoid(t, dim).double()).abs().max()) <= 2e-3            # sin / cos of ~1e3 rad from an fp32 argument
        assert truth.shape == (len(SR.TS_T), dim) and float(a.max()) == 1000.0
    x = torch.linspace(-30, 30, 4001, dtype=F64)
    assert float((SR.gelu64(x) - torch.nn.functional.gelu(x, approximate="tanh")).abs().max()) <= 1e-14
    for c in SR.LINEAR_CASES:
        xx, W, b, Rr = SR.linear_data(c)
        want = torch.nn.functional.linear(torch.nn.functional.silu(xx.double()) if c[8] else xx.double(), W.double(), None if b is None else b.double())
        want = want if Rr is None else want + Rr.double()
        assert float(SR.row_rel(SR.small_linear64(xx, W, b, Rr, c[8]), want).max()) <= 1e-14


def _torch_adamw(case, p0, g_eff32, steps=2):
    """torch.optim.AdamW(foreach=False) in the given dtype on the case's tensors, one optimizer per hyper-parameter group -> per step (p, m, v)"""
    ps = [torch.nn.Parameter(p.to(g_eff32[0][i].dtype).clone()) for i, p in enumerate(p0)]
    opts = [torch.optim.AdamW([p for p, t in zip(ps, case) if t["group"] == k], lr=gr["lr"], weight_decay=gr["wd"], betas=gr["betas"], eps=gr["eps"],
                              foreach=False) for k, gr in enumerate(SR.OPT_GROUPS)]
    out = []
    for s in range(steps):
        for p, g in zip(ps, g_eff32[s]):
            p.grad = g.clone()
        for o in opts:
            o.step()
        st = [next(o.state[p] for o in opts if p in o.state) if p.numel() or any(p in o.state for o in opts) else None for p in ps]
        out.append(([p.detach().clone() for p in ps], [x["exp_avg"].clone() for x in st], [x["exp_avg_sq"].clone() for x in st]))
    return out


def _clipped(grads_step):
    truth = float(torch.cat([g.to(F64) for g in grads_step]).norm())
    coef = SR.f32(SR.clip_coef64(truth, SR.OPT_MAX_NORM))
    return [(g.float() * torch.tensor(coef, dtype=F32)) for g in grads_step]


def test_adamw_reference_equals_torch_fp64():
    case = [t for t in SR.optim_case("aligned") if t["n"] <= 9]
    p0, grads = SR.optim_data(case, 0)
    g64 = [[g.double() for g in gs] for gs in grads]
    tor = _torch_adamw(case, p0, g64)
    ref = SR.AdamWRef64(p0)
    for s in range(2):
        ref.step(g64[s], *SR.optim_hyper(case))
        for i in range(len(case)):
            for a, b in ((ref.p[i], tor[s][0][i]), (ref.m[i], tor[s][1][i]), (ref.v[i], tor[s][2][i])):
                assert float((a - b).abs().max() if a.numel() else 0.0) <= 1e-15 + 4e-16 * float(b.abs().max() if b.numel() else 0.0), (s, i)
    n32 = torch.tensor(12.345678, dtype=F32)
    assert abs(float(SR.clip_coef32(n32, 1.0)) - SR.clip_coef64(float(n32), 1.0)) <= 1e-7 and SR.clip_coef64(0.5, 1.0) == 1.0
    assert float(SR.clip_coef32(torch.tensor(float("inf")), 1.0)) == 0.0


# ----------------------------------------------------------------------------------------------------------------------------------
# the recorded torch figures
# ----------------------------------------------------------------------------------------------------------------------------------
def _recorded(name, measured, recorded):
    print(f"{name}: torch fp32 measured {measured:.4g}, recorded {recorded:.4g}")
    assert recorded / 2 <= measured <= recorded, (name, measured, recorded)


def test_recorded_torch_figures():
    c_ts = 0.0
    for c in SR.TS_CASES:
        t = SR.ts_times(c)
        truth, a = SR.timestep_embed64(t, c["dim"])
        c_ts = max(c_ts, float(((SR.timestep_embed_torch32(t, c["dim"]).double() - truth).abs() / (SR.EPS32 * a.clamp_min(1.0))).max()))
    _recorded("timestep_embed c", c_ts, SR.TS_C_TORCH)
    # the guidance-sized arguments (up to 29952): torch's constant there is within the recorded one, so TS_GUIDANCE_CASES use the same bound
    c_gd = 0.0
    for c in SR.TS_GUIDANCE_CASES:
        t = SR.ts_times(c)
        truth, a = SR.timestep_embed64(t, c["dim"])
        c_gd = max(c_gd, float(((SR.timestep_embed_torch32(t, c["dim"]).double() - truth).abs() / (SR.EPS32 * a.clamp_min(1.0))).max()))
    _recorded("timestep_embed c at guidance arguments", c_gd, SR.TS_C_TORCH)
    c_g = 0.0
    for c in SR.flat_cases("gelu"):
        x, _ = SR.flat_data(c, F32, big=True)
        c_g = max(c_g, float(((SR.gelu_torch32(x).double() - SR.gelu64(x)).abs() / (SR.EPS32 * x.double().abs())).max()))
    _recorded("gelu_tanh c", c_g, SR.GELU_C_TORCH)
    r = 0.0
    for c in SR.LINEAR_CASES:
        x, W, b, Rr = SR.linear_data(c)
        r = max(r, float(SR.row_rel(SR.small_linear_torch32(x, W, b, Rr, c[8]).double(), SR.small_linear64(x, W, b, Rr, c[8])).max()))
    _recorded("small_linear per-row", r, SR.LINEAR_ROW_TORCH)


def test_recorded_torch_adamw_figure():
    k = 0.0
    for mode in SR.OPT_MODES[:3]:                      # the data depends on the mode only through its seed
        for clip in (False, True):
            case = SR.optim_case(mode)
            p0, grads = SR.optim_data(case, SR.OPT_MODES.index(mode))
            g32 = [_clipped(gs) if clip else [g.float() for g in gs] for gs in grads]
            tor = _torch_adamw(case, p0, g32)
            ref = SR.AdamWRef64(p0)
            for s in range(2):
                ref.step([g.double() for g in g32[s]], *SR.optim_hyper(case))
                for i, t in enumerate(case):
                    if t["n"] == 0:
                        continue
                    for got, truth, scale in ((tor[s][0][i], ref.p[i], ref.scale_p[i]), (tor[s][1][i], ref.m[i], ref.scale_m[i]), (tor[s][2][i], ref.v[i], ref.scale_v[i])):
                        k = max(k, float(((got.double() - truth).abs() / (2.0 ** -23 * scale).clamp_min(1e-300)).max()))
    _recorded("AdamW k", k, SR.ADAMW_K_TORCH)


# ----------------------------------------------------------------------------------------------------------------------------------
# preconditions: no generator emits a case the kernel documents as refused; the refusal tables are refusals
# ----------------------------------------------------------------------------------------------------------------------------------
def test_cases_meet_the_documented_preconditions():
    for kind in ("euler", "cfg"):
        cs = SR.flat_cases(kind)
        assert all(SR.flat_check(c["n"], c["off"], es) == SR.OK for c in cs for es in (2, 4)) and {c["n"] for c in cs} >= set(SR.FLAT_N)
        assert max(c["n"] for c in cs) > SR.GRID_ELEMS            # the grid-stride loop runs twice
    assert {c["gs"] for c in SR.flat_cases("cfg")} == set(SR.CFG_GS) and {c["dt"] for c in SR.flat_cases("euler")} == set(SR.EULER_DT)
    ge = SR.flat_cases("gelu")
    assert any(c["n"] % 8 for c in ge) and any(c["off"] == 1 for c in ge) and all(c["n"] > 0 for c in ge)
    assert all(SR.flat_check(r["n"], r["off"], 2) == r["code"] != SR.OK for r in SR.FLAT_REFUSED)
    for kind in ("add", "rowbcast", "gather", "gate"):
        cs = SR.row_cases(kind)
        assert {c["rows"] for c in cs} == set(SR.ROWS) and {c["D"] for c in cs} == set(SR.DS)
        for c in cs:
            assert SR.row_check(c["D"], (c["ld_a"], c["ld_b"], c["ld_o"], c["ld_x"])) == SR.OK and min(c["ld_a"], c["ld_b"], c["ld_o"], c["ld_x"]) >= c["D"]
        assert {c[k] - c["D"] for c in cs for k in ("ld_a", "ld_o")} == set(SR.LD_EXTRA)
        assert any(len({c["ld_a"], c["ld_b"], c["ld_o"]}) == 3 for c in cs)
    rb = SR.row_cases("rowbcast")
    assert any(c["rpb"] == 1 for c in rb) and any(c["rpb"] == c["rows"] > 1 for c in rb) and any(1 < c["rpb"] < c["rows"] and c["rows"] % c["rpb"] == 0 for c in rb)
    assert any(c["rows"] % c["rpb"] for c in rb) and all(c["rpb"] > 0 for c in rb)
    ga = SR.row_cases("gate")
    assert {c["x"] for c in ga} == {"none", "given", "alias"} and any(c["rows"] % c["rps"] for c in ga) and any(1 < c["rps"] < c["rows"] and c["rows"] % c["rps"] == 0 for c in ga)
    assert {c["idx"] for c in SR.row_cases("gather")} == {"mixed", "all_negative", "duplicates", "last_row"}
    for c in SR.row_cases("gather"):
        idx = SR.gather_idx(c, torch.Generator().manual_seed(0))
        assert int(idx.max()) < c["src_rows"] and idx.shape == (c["rows"],)
    assert all(SR.row_check(r["D"], (r["ld"],), (r["off"],), 2) == SR.BAD_ALIGN for r in SR.ROW_REFUSED)
    assert all(SR.pack_check(*s) == SR.OK for s in SR.PACK_CASES) and all(SR.pack_check(*s) == SR.BAD_SHAPE for s in SR.PACK_REFUSED)
    assert any(s[1] == 1 for s in SR.PACK_CASES) and any(s[1] == 16 for s in SR.PACK_CASES) and (2, 16, 128, 128) in SR.PACK_CASES
    for b, r, c, p, es, ed, eb in SR.TRANSPOSE_CASES:
        assert SR.transpose_check(r, c, p, c + es, p + ed) == SR.OK and b < 65536 and (p + 63) // 64 < 65536
    assert {p - r for _, r, _, p, *_ in SR.TRANSPOSE_CASES} >= {0, 1, 7, 8, 63} and {c for _, _, c, *_ in SR.TRANSPOSE_CASES} >= {8, 72, 130}
    assert all(c["B"] > 0 and c["dim"] % 2 == 0 and c["dim"] > 0 for c in SR.TS_CASES) and {c["dim"] for c in SR.TS_CASES} == {2, 64, 256, 320, 1024}
    assert all(set(SR.ts_times(c).tolist()[:6]) <= {SR.f32(v) for v in SR.TS_T} for c in SR.TS_CASES)
    assert {(c["B"], c["dim"]) for c in SR.TS_GUIDANCE_CASES} == {(1, 256), (5, 256)} and any(c["slack"] for c in SR.TS_GUIDANCE_CASES)
    want = [float(torch.tensor(g, dtype=SR.BF) * 1000) for g in SR.TS_GUIDANCE]
    assert want == [1000.0, 3504.0, 7008.0, 29952.0] and SR.ts_times(SR.TS_GUIDANCE_CASES[0]).tolist() == want[-1:]
    assert all(set(SR.ts_times(c).tolist()) == set(want) for c in SR.TS_GUIDANCE_CASES if c["B"] >= 4)
    assert all(0 < c[0] <= 64 and c[1] > 0 and c[2] > 0 for c in SR.LINEAR_CASES)
    hs = set()
    for mode in SR.OPT_MODES:
        case = SR.optim_case(mode)
        assert {t["n"] for t in case} == set(SR.OPT_NUMEL) and {(t["gbf"], t["master"]) for t in case} == set(SR.OPT_FORMS) and {t["group"] for t in case} == {0, 1}
        assert all(0 <= o <= 8 for t in case for o in t["off"].values())
        hs |= {t["h"] for t in case if t["n"] == SR.CHUNK + 1}
        if mode == "odd_param":                            # no common aligned element: every chunk is scalar
            assert all(t["h"] == min(t["n"], SR.CHUNK) for t in case)
        if mode[0] == "h":
            assert all(t["h"] == min(int(mode[1:]), t["n"]) for t in case if t["gbf"] or t["master"] or int(mode[1:]) < 4), mode
    assert {0, 1, 3, 7, SR.CHUNK} <= hs
    assert SR.regions(20, 3).tolist() == [0] * 3 + [1] * 16 + [2] and SR.regions(5, 5).tolist() == [0] * 5
    r = SR.regions(SR.CHUNK + 9, 7)
    assert r[SR.CHUNK:].tolist() == [0] * 7 + [2] * 2 and int((r[:SR.CHUNK] == 1).sum()) == (SR.CHUNK - 7) // 8 * 8


# ----------------------------------------------------------------------------------------------------------------------------------
# mutation checks
# ----------------------------------------------------------------------------------------------------------------------------------
def _image_slips(before_image, want_image, mask):
    """the output-shaped slips: the last vector chunk skipped, the first elements skipped, one element past the end written"""
    idx = torch.nonzero(mask).flatten()
    out = {}
    a = want_image.clone(); a[idx[-8:]] = before_image[idx[-8:]]; out["tail chunk skipped"] = a
    a = want_image.clone(); a[idx[:3]] = before_image[idx[:3]]; out["head elements skipped"] = a
    a = want_image.clone(); a[idx[-1] + 1] = want_image[idx[-1]]; out["one element past the end written"] = a
    a = want_image.clone(); a[idx[0] - 1] = want_image[idx[0]]; out["one element before the start written"] = a
    return out


@pytest.mark.parametrize("dt", DTS)
def test_mutations_flat_ops(dt):
    c = dict(n=4104, seed=3, off=0)
    x, v = SR.flat_data(c, dt)
    mask = _flat_mask(c["n"])
    for name, fn, slips in (("euler", lambda s=None: SR.euler_step(x, v, -0.0132729, s), ["product_unrounded"] + (["dt_unrounded"] if dt == BF else [])),
                            ("cfg", lambda s=None: SR.cfg_combine(x, v, 3.5, s), ["product_unrounded", "difference_unrounded"])):
        want = _image(fn(), mask, dt)
        SR.judge_exact(name, want, want, mask)
        before = _image(x, mask, dt) if name == "euler" else torch.full(mask.shape, SR.SENT, dtype=dt)
        for k, img in _image_slips(before, want, mask).items():
            _rejects(lambda: SR.judge_exact(f"{name}: {k}", img, want, mask))
        if dt == BF:                                       # a dropped rounding point is invisible in the fp32 twin by definition: it rounds to fp32 only
            for s in slips:
                _rejects(lambda: SR.judge_exact(f"{name}: {s}", _image(fn(s), mask, dt), want, mask))
    xg, _ = SR.flat_data(c, dt, big=True)
    truth = SR.gelu64(xg)
    bound = SR.gelu_bound(xg, truth, dt)
    good = _image(SR.gelu_torch32(xg.float()) if dt == F32 else truth, mask, dt)
    SR.judge_bounded("gelu", good, truth, bound, mask)
    for k, img in _image_slips(torch.full(mask.shape, SR.SENT, dtype=dt), good, mask).items():
        _rejects(lambda: SR.judge_bounded(f"gelu: {k}", img, truth, bound, mask))
    erf = _image(torch.nn.functional.gelu(xg.float()), mask, dt)                       # the erf GELU for the tanh one
    _rejects(lambda: SR.judge_bounded("gelu: erf form", erf, truth, bound, mask))
    if dt == F32:
        _rejects(lambda: SR.judge_bounded("gelu: a bf16-rounded result in the fp32 twin", _image(truth.to(BF), mask, dt), truth, bound, mask))


@pytest.mark.parametrize("dt", DTS)
def test_mutations_row_ops(dt):
    g = torch.Generator().manual_seed(5)
    rows, D, ld, rp = 37, 64, 72, 5
    a, b = SR.mags(g, (rows, D)).to(dt), SR.mags(g, (rows, D)).to(dt)
    tab, gate = SR.mags(g, (rp, D)), SR.mags(g, ((rows + rp - 1) // rp, D), -2, 1).to(dt)
    _, _, mask = SR.guarded(rows, D, ld, dt)
    sent = torch.full(mask.shape, SR.SENT, dtype=dt)
    src, idx = SR.mags(g, (9, D)).to(dt), torch.tensor(([3, -1, 8, 0, 3, -2, 7] * 6)[:rows], dtype=torch.int32)
    ops = {"add": (lambda s=None: SR.add(a, b), sent, []),
           "rowbcast": (lambda s=None: SR.add_rowbcast(a, tab, rp, s), _image(a, mask, dt), ["row_not_wrapped"]),
           "gate": (lambda s=None: SR.gate_residual(b, a, gate, rp, s), sent, ["sample_is_remainder"] + (["product_unrounded"] if dt == BF else [])),
           "gather": (lambda s=None: SR.gather_rows(src, idx, s), sent, ["negative_reads_row_0"])}
    for name, (fn, before, slips) in ops.items():
        want = _image(fn(), mask, dt)
        SR.judge_exact(name, want, want, mask)
        for k, img in _image_slips(before, want, mask).items():
            _rejects(lambda: SR.judge_exact(f"{name}: {k}", img, want, mask))
        for s in slips:
            _rejects(lambda: SR.judge_exact(f"{name}: {s}", _image(fn(s), mask, dt), want, mask))
        # the row stride confused with D: the same values written densely from the view's start
        dense = torch.full(mask.shape, SR.SENT, dtype=dt)
        dense[SR.GUARD:SR.GUARD + rows * D] = fn().reshape(-1)
        _rejects(lambda: SR.judge_exact(f"{name}: row stride confused with D", dense, want, mask))
        last = want.clone()
        last[torch.nonzero(mask).flatten()[-D:]] = before[torch.nonzero(mask).flatten()[-D:]]
        _rejects(lambda: SR.judge_exact(f"{name}: last row skipped", last, want, mask))


def test_mutations_pack_transpose_timestep_linear():
    g = torch.Generator().manual_seed(6)
    lat = torch.randn(2, 3, 6, 10, generator=g).to(BF)
    mask = _flat_mask(lat.numel())
    want = _image(SR.pack_latents(lat), mask, BF)
    SR.judge_exact("pack", want, want, mask)
    _rejects(lambda: SR.judge_exact("pack: dy / dx swapped", _image(SR.pack_latents(lat, "dy_dx_swapped"), mask, BF), want, mask))
    packed = SR.pack_latents(lat)
    _rejects(lambda: SR.judge_exact("unpack: dy / dx swapped", _image(SR.unpack_latents(packed, 6, 10, "dy_dx_swapped"), mask, BF), _image(lat, mask, BF), mask))
    _rejects(lambda: SR.judge_exact("pack: H and W exchanged", _image(SR.pack_latents(lat.reshape(2, 3, 10, 6)), mask, BF), want, mask))
    src = torch.randn(2, 57, 8, generator=g).to(BF)
    tm = _flat_mask(2 * 8 * 64)
    wt = _image(SR.transpose(src, 64), tm, BF)
    SR.judge_exact("transpose", wt, wt, tm)
    _rejects(lambda: SR.judge_exact("transpose: pad columns left unwritten", _image(SR.transpose(src, 64, fill=SR.SENT), tm, BF), wt, tm))
    for k, img in _image_slips(torch.full(tm.shape, SR.SENT, dtype=BF), wt, tm).items():
        _rejects(lambda: SR.judge_exact(f"transpose: {k}", img, wt, tm))
    for dt in DTS:
        c = SR.TS_CASES[4]
        t = SR.ts_times(c)
        truth, a = SR.timestep_embed64(t, c["dim"])
        _, _, m = SR.guarded(c["B"], c["dim"], c["dim"] + c["slack"], dt)
        bound = SR.timestep_bound(a, truth, dt)
        good = _image(SR.timestep_embed_torch32(t, c["dim"]), m, dt)
        SR.judge_bounded("timestep", good, truth, bound, m)
        half = c["dim"] // 2
        swapped = torch.cat([truth[:, half:], truth[:, :half]], 1)
        _rejects(lambda: SR.judge_bounded("timestep: [sin | cos]", _image(swapped, m, dt), truth, bound, m))
        shifted, _ = SR.timestep_embed64(t * (1 + 2.0 ** -17), c["dim"])                       # an argument 64 fp32 roundings off
        _rejects(lambda: SR.judge_bounded("timestep: argument rounded to 18 bits", _image(shifted, m, dt), truth, bound, m))
        f1 = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / (half - 1))            # downscale_freq_shift = 1
        a1 = t.double()[:, None] * f1
        _rejects(lambda: SR.judge_bounded("timestep: freq shift 1", _image(torch.cat([a1.cos(), a1.sin()], 1), m, dt), truth, bound, m))
        for k, img in _image_slips(torch.full(m.shape, SR.SENT, dtype=dt), good, m).items():
            _rejects(lambda: SR.judge_bounded(f"timestep: {k}", img, truth, bound, m))
        # guidance-sized arguments: the same bound accepts torch's fp32 evaluation and still separates the slips below at |t f| up to 29952
        c = SR.TS_GUIDANCE_CASES[2]
        t = SR.ts_times(c)
        truth, a = SR.timestep_embed64(t, c["dim"])
        _, _, m = SR.guarded(c["B"], c["dim"], c["dim"] + c["slack"], dt)
        bound = SR.timestep_bound(a, truth, dt)
        SR.judge_bounded("timestep, guidance", _image(SR.timestep_embed_torch32(t, c["dim"]), m, dt), truth, bound, m)
        shifted, _ = SR.timestep_embed64(t * (1 + 2.0 ** -17), c["dim"])
        _rejects(lambda: SR.judge_bounded("timestep, guidance: argument rounded to 18 bits", _image(shifted, m, dt), truth, bound, m))
        plain, _ = SR.timestep_embed64(torch.tensor([1000.0 * g_ for g_ in (SR.TS_GUIDANCE[::-1] * 2)[:c["B"]]], dtype=F32), c["dim"])
        _rejects(lambda: SR.judge_bounded("timestep, guidance: the scale not rounded to bf16 (3500, 7000, 30000)", _image(plain, m, dt), truth, bound, m))
    c = SR.LINEAR_CASES[1]
    x, W, b, Rr = SR.linear_data(c)
    truth = SR.small_linear64(x, W, b, Rr, True)
    bound = SR.LINEAR_MARGIN * SR.LINEAR_ROW_TORCH
    SR.judge_rows("linear", SR.small_linear_torch32(x, W, b, Rr, True).double(), truth, bound)
    _rejects(lambda: SR.judge_rows("linear: SiLU dropped", SR.small_linear64(x, W, b, Rr, False), truth, bound))
    _rejects(lambda: SR.judge_rows("linear: residual dropped", SR.small_linear64(x, W, b, None, True), truth, bound))
    _rejects(lambda: SR.judge_rows("linear: the last 4 of K dropped", SR.small_linear64(x[:, :-4], W[:, :-4], b, Rr, True), truth, bound))
    lastrow = truth.clone(); lastrow[-1] = truth[-2]
    _rejects(lambda: SR.judge_rows("linear: last row wrong", lastrow, truth, bound))
    onecol = truth.clone(); onecol[2, -1] = 0.0                                        # the last column of one row: invisible to a global rel-L2 of 1e-3
    _rejects(lambda: SR.judge_rows("linear: last column of a row unwritten", onecol, truth, bound))


def test_mutations_optimizer():
    case = [t for t in SR.optim_case("h7") if t["n"] in (9, 65537)]
    p0, grads = SR.optim_data(case, 4)
    hyper = SR.optim_hyper(case)
    g64 = [[g.double() for g in gs] for gs in grads]

    def run(slip=None, steps=2):
        r = SR.AdamWRef64(p0)
        for s in range(steps):
            r.step(g64[s], *hyper, slip=slip)
        return r

    ref = run()
    tor = _torch_adamw(case, p0, [[g.float() for g in gs] for gs in grads])[1]

    def judge(name, ps, ms, vs):
        for i, t in enumerate(case):
            mask, reg = _flat_mask(t["n"], t["off"]["exp_avg"]), SR.regions(t["n"], t["h"])
            for what, got, truth, scale in (("p", ps[i], ref.p[i], ref.scale_p[i]), ("m", ms[i], ref.m[i], ref.scale_m[i]), ("v", vs[i], ref.v[i], ref.scale_v[i])):
                SR.judge_bounded(f"{name} tensor {i} {what}", _image(got, mask, F32), truth, SR.adamw_bound(scale), mask, reg)

    judge("torch fp32", *tor)
    for slip in ("lerp_swapped", "bias_correction_of_previous_step"):
        bad = run(slip)
        _rejects(lambda: judge(slip, bad.p, bad.m, bad.v))
    one = run(steps=1)                                      # regions: an element of the head / the tail that missed step 2 (a global rel-L2 would pass it)
    for where, k in (("head", 0), ("head", 6), ("body", 7), ("tail", 65535)):
        ps = [p.clone() for p in ref.p]
        i = next(j for j, t in enumerate(case) if t["n"] == 65537)
        ps[i][k] = one.p[i][k]
        assert SR.REGION_NAMES[int(SR.regions(65537, 7)[k])] == where
        with pytest.raises(AssertionError, match=where):
            judge(f"{where} element {k} not updated", ps, ref.m, ref.v)
        rel = float((torch.cat(ps) - torch.cat(ref.p)).norm() / torch.cat(ref.p).norm())
        assert rel < 1e-4                                   # what the concatenated rel-L2 of the older tests would have seen
    for dt in DTS:
        gq = grads[0][0].to(dt)
        mask = _flat_mask(gq.numel(), 3)
        want = _image(SR.grad_scale(gq, 0.0123456), mask, dt)
        SR.judge_exact("grad_scale", want, want, mask)
        for k, img in _image_slips(_image(gq, mask, dt), want, mask).items():
            _rejects(lambda: SR.judge_exact(f"grad_scale: {k}", img, want, mask))
    master = (p0[-1] * 1.001).contiguous()                 # not bf16-representable
    pm = _flat_mask(master.numel())
    trunc = master.view(torch.int32).bitwise_and(-65536).view(F32)
    _rejects(lambda: SR.judge_exact("bf16 param: master truncated, not rounded to nearest even", _image(trunc, pm, BF), _image(master.to(BF), pm, BF), pm))
