"""Sweep of the step, glue and optimizer kernels (csrc/elementwise.hip: timestep_embed, euler_step, cfg_combine, add, add_rowbcast, gather_rows,
pack / unpack_latents, small_linear_f32; csrc/backward.hip: gate_residual, gelu_tanh forward, transpose; csrc/optim.hip) against the float64
references and case tables of tests/step_kernel_ref.py, which tests/test_step_kernel_ref_cpu.py pins to torch and the oracle.

What is asserted (docs/PARITY_TOLERANCES.md, "Step / glue / optimizer kernel sweep"):
  - euler_step, cfg_combine, add, add_rowbcast, gate_residual, grad_scale, gather_rows, pack / unpack, transpose: BIT equality with the reference,
    in bf16 and in the fp32 twin, on every case;
  - timestep_embed / gelu_tanh: a per-element bound against fp64 truth, 4 x torch's own fp32 error on the same cases (+ half a bf16 ulp for bf16);
  - small_linear_f32: per-row relative error <= 4 x torch's F.linear on the same cases;
  - AdamW: every element of param / master / exp_avg / exp_avg_sq within 2 x torch's own fp32 AdamW error of the fp64 recurrence after steps 1 and
    2, head / body / tail of every chunk reported separately; bf16 params equal to bf16(master); the norm within 1e-6 of fp64, the clip coefficient
    bit-equal to torch's fp32 formula on the kernel's norm.
Every output sits in a buffer of sentinels (before, after, and between the rows of a strided output) that must come back untouched; read-only
operands are compared with their clones; refused argument sets must return their documented code and write nothing. Every case runs: nothing is
skipped or filtered. All calls go straight to the C ABI (unigen_amd.lib), so that strides, offsets and descriptor forms the Python host never
produces are reached."""
import ctypes as C

import pytest
import torch

from tests import step_kernel_ref as SR

pytestmark = pytest.mark.gpu
BF, F32, F64 = SR.BF, SR.F32, SR.F64
G = SR.GUARD
TWIN = {"ug_add_bf16": "ug_add_f32", "ug_add_rowbcast_f32": "ug_add_rowbcast_f32_f32"}
DTS = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
_ids = lambda cases: [c["id"] for c in cases]


def _fn(name, dt):
    from unigen_amd import lib as L
    return getattr(L.load(), name if dt == BF else TWIN.get(name, name + "_f32"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _flat(n, off, dt, dev, values=None):
    """-> (device buffer of sentinels with `values` at [G + off, G + off + n), that slice, the CPU mask of the slice)"""
    buf = torch.full((G + off + n + G,), SR.SENT, dtype=dt)
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[G + off:G + off + n] = True
    if values is not None:
        buf[mask] = values.to(dt)
    d = buf.to(dev)
    assert d.data_ptr() % 16 == 0
    return d, d[G + off:G + off + n], mask


def _rows(rows, D, ld, dt, dev, values=None):
    """a [rows, D] view with leading dimension ld in a device buffer of sentinels (the columns [D, ld) of each row are sentinels too)"""
    buf, view, mask = SR.guarded(rows, D, ld, dt)
    if values is not None:
        view.copy_(values)
    d = buf.to(dev)
    assert d.data_ptr() % 16 == 0
    return d, d[G:G + rows * ld].view(rows, ld)[:, :D], mask


def _operand(rows, D, ld, dt, dev, values):
    """a read-only [rows, D] operand with leading dimension ld -> (device view, device clone of its whole buffer)"""
    full = torch.zeros(rows, ld, dtype=dt)
    full[:, :D] = values
    d = full.to(dev)
    return d[:, :D], d.clone(), d


def _image(want_values, mask, dt):
    img = torch.full(mask.shape, SR.SENT, dtype=dt)
    img[mask] = want_values.reshape(-1)
    return img


def _sync_cpu(t):
    torch.cuda.synchronize()
    return t.cpu()


# ----------------------------------------------------------------------------------------------------------------------------------
# flat ops
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.flat_cases("euler"), ids=_ids(SR.flat_cases("euler")))
def test_euler_step(gpu, c, dt):
    assert SR.flat_check(c["n"], 0, 2 if dt == BF else 4) == SR.OK
    x, v = SR.flat_data(c, dt)
    xb, xs, mask = _flat(c["n"], 0, dt, gpu, x)
    vd = v.to(gpu)
    v0 = vd.clone()
    assert _fn("ug_euler_step", dt)(xs.data_ptr(), vd.data_ptr(), c["dt"], c["n"], _stream()) == 0
    SR.judge_exact(f"euler_step {c['id']}", _sync_cpu(xb), _image(SR.euler_step(x, v, c["dt"]), mask, dt), mask)
    assert torch.equal(vd, v0), "v was written"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.flat_cases("cfg"), ids=_ids(SR.flat_cases("cfg")))
def test_cfg_combine(gpu, c, dt):
    assert SR.flat_check(c["n"], 0, 2 if dt == BF else 4) == SR.OK
    u, t = SR.flat_data(c, dt)
    ob, os_, mask = _flat(c["n"], 0, dt, gpu)
    ud, td = u.to(gpu), t.to(gpu)
    u0, t0 = ud.clone(), td.clone()
    assert _fn("ug_cfg_combine", dt)(ud.data_ptr(), td.data_ptr(), c["gs"], os_.data_ptr(), c["n"], _stream()) == 0
    SR.judge_exact(f"cfg_combine {c['id']}", _sync_cpu(ob), _image(SR.cfg_combine(u, t, c["gs"]), mask, dt), mask)
    assert torch.equal(ud, u0) and torch.equal(td, t0), "uncond / text were written"


@pytest.mark.parametrize("dt", DTS)
def test_flat_refusals(gpu, dt):
    """n % 8 != 0 or a base off 16 bytes: UG_ERR_BAD_ALIGN from euler_step and cfg_combine, nothing written"""
    es = 2 if dt == BF else 4
    for r in SR.FLAT_REFUSED:
        if SR.flat_check(r["n"], r["off"], es) == SR.OK:           # an offset of 4 fp32 elements is 16 bytes: not a refusal for the twin
            continue
        assert SR.flat_check(r["n"], r["off"], es) == r["code"]
        xb, xs, _ = _flat(r["n"], r["off"], dt, gpu)
        ob, os_, _ = _flat(r["n"], r["off"], dt, gpu)
        assert _fn("ug_euler_step", dt)(xs.data_ptr(), os_.data_ptr(), -0.25, r["n"], _stream()) == r["code"], r
        assert _fn("ug_cfg_combine", dt)(xs.data_ptr(), xs.data_ptr(), 3.5, os_.data_ptr(), r["n"], _stream()) == r["code"], r
        assert bool((_sync_cpu(xb) == SR.SENT).all() and (ob.cpu() == SR.SENT).all()), ("a refused call wrote", r)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.flat_cases("gelu"), ids=_ids(SR.flat_cases("gelu")))
def test_gelu_tanh_forward(gpu, c, dt):
    x, _ = SR.flat_data(c, dt, big=True)
    xb, xs, _ = _flat(c["n"], c["off"], dt, gpu, x)
    x0 = xb.clone()
    yb, ys, mask = _flat(c["n"], c["off"], dt, gpu)
    assert _fn("ug_gelu_tanh", dt)(xs.data_ptr(), ys.data_ptr(), c["n"], _stream()) == 0
    truth = SR.gelu64(x)
    w = SR.judge_bounded(f"gelu_tanh {c['id']}", _sync_cpu(yb), truth, SR.gelu_bound(x, truth, dt), mask)
    if dt == F32:
        got = yb.cpu()[mask].to(F64)
        ck = float(((got - truth).abs() / (SR.EPS32 * x.to(F64).abs())).max())
        print(f"gelu_tanh_f32 {c['id']}: kernel c = {ck:.2f} (torch {SR.GELU_C_TORCH}, bound {SR.GELU_MARGIN * SR.GELU_C_TORCH})")
    else:
        print(f"gelu_tanh bf16 {c['id']}: worst |err| / bound = {w['all']:.3f}")
    assert torch.equal(xb, x0), "x was written"


# ----------------------------------------------------------------------------------------------------------------------------------
# row ops
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.row_cases("add"), ids=_ids(SR.row_cases("add")))
def test_add(gpu, c, dt):
    rows, D = c["rows"], c["D"]
    assert SR.row_check(D, (c["ld_a"], c["ld_b"], c["ld_o"])) == SR.OK
    g = torch.Generator().manual_seed(2000 + c["seed"])
    a, b = SR.mags(g, (rows, D)).to(dt), SR.mags(g, (rows, D)).to(dt)
    av, a0, af = _operand(rows, D, c["ld_a"], dt, gpu, a)
    bv, b0, bfull = _operand(rows, D, c["ld_b"], dt, gpu, b)
    ob, ov, mask = _rows(rows, D, c["ld_o"], dt, gpu)
    assert _fn("ug_add_bf16", dt)(av.data_ptr(), c["ld_a"], bv.data_ptr(), c["ld_b"], ov.data_ptr(), c["ld_o"], rows, D, _stream()) == 0
    SR.judge_exact(f"add {c['id']}", _sync_cpu(ob), _image(SR.add(a, b), mask, dt), mask)
    assert torch.equal(af, a0) and torch.equal(bfull, b0), "an operand was written"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.row_cases("rowbcast"), ids=_ids(SR.row_cases("rowbcast")))
def test_add_rowbcast(gpu, c, dt):
    rows, D, rpb = c["rows"], c["D"], c["rpb"]
    assert SR.row_check(D, (c["ld_x"], c["ld_a"])) == SR.OK
    g = torch.Generator().manual_seed(2100 + c["seed"])
    x, tab = SR.mags(g, (rows, D)).to(dt), SR.mags(g, (min(rows, rpb), D))
    tv, t0, tf = _operand(tab.shape[0], D, c["ld_a"], F32, gpu, tab)
    xb, xv, mask = _rows(rows, D, c["ld_x"], dt, gpu, x)
    assert _fn("ug_add_rowbcast_f32", dt)(xv.data_ptr(), c["ld_x"], tv.data_ptr(), c["ld_a"], rows, rpb, D, _stream()) == 0
    SR.judge_exact(f"add_rowbcast {c['id']}", _sync_cpu(xb), _image(SR.add_rowbcast(x, tab, rpb), mask, dt), mask)
    assert torch.equal(tf, t0), "the table was written"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.row_cases("gate"), ids=_ids(SR.row_cases("gate")))
def test_gate_residual(gpu, c, dt):
    rows, D, rps = c["rows"], c["D"], c["rps"]
    assert SR.row_check(D, (c["ld_x"], c["ld_a"], c["ld_b"], c["ld_o"])) == SR.OK
    g = torch.Generator().manual_seed(2200 + c["seed"])
    samples = (rows + rps - 1) // rps
    a, gate, x = SR.mags(g, (rows, D), -2, 2).to(dt), SR.mags(g, (samples, D), -2, 1).to(dt), SR.mags(g, (rows, D)).to(dt)
    av, a0, af = _operand(rows, D, c["ld_a"], dt, gpu, a)
    gv, g0, gf = _operand(samples, D, c["ld_b"], dt, gpu, gate)
    if c["x"] == "alias":                                   # y aliased to x: the output buffer holds x
        yb, yv, mask = _rows(rows, D, c["ld_o"], dt, gpu, x)
        xp, ldx = yv.data_ptr(), c["ld_o"]
    else:
        yb, yv, mask = _rows(rows, D, c["ld_o"], dt, gpu)
        xv, x0, xf = _operand(rows, D, c["ld_x"], dt, gpu, x)
        xp, ldx = (xv.data_ptr(), c["ld_x"]) if c["x"] == "given" else (None, 0)
    assert _fn("ug_gate_residual", dt)(xp, ldx, av.data_ptr(), c["ld_a"], gv.data_ptr(), c["ld_b"], rps, yv.data_ptr(), c["ld_o"], rows, D, _stream()) == 0
    want = SR.gate_residual(None if c["x"] == "none" else x, a, gate, rps)
    SR.judge_exact(f"gate_residual {c['id']}", _sync_cpu(yb), _image(want, mask, dt), mask)
    assert torch.equal(af, a0) and torch.equal(gf, g0) and (c["x"] == "alias" or torch.equal(xf, x0)), "an operand was written"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.row_cases("gather"), ids=_ids(SR.row_cases("gather")))
def test_gather_rows(gpu, c, dt):
    rows, D = c["rows"], c["D"]
    assert SR.row_check(D, (c["ld_a"], c["ld_o"])) == SR.OK
    g = torch.Generator().manual_seed(2300 + c["seed"])
    src, idx = SR.mags(g, (c["src_rows"], D)).to(dt), SR.gather_idx(c, g)
    sv, s0, sf = _operand(c["src_rows"], D, c["ld_a"], dt, gpu, src)
    ob, ov, mask = _rows(rows, D, c["ld_o"], dt, gpu)
    idxd = idx.to(gpu)
    assert _fn("ug_gather_rows", dt)(sv.data_ptr(), c["ld_a"], idxd.data_ptr(), ov.data_ptr(), c["ld_o"], rows, D, _stream()) == 0
    SR.judge_exact(f"gather_rows {c['id']}", _sync_cpu(ob), _image(SR.gather_rows(src, idx), mask, dt), mask)
    assert torch.equal(sf, s0), "the source was written"


@pytest.mark.parametrize("dt", DTS)
def test_row_refusals(gpu, dt):
    """D or a leading dimension that is no multiple of 8, or a base off 16 bytes: UG_ERR_BAD_ALIGN from the four row ops, nothing written"""
    es = 2 if dt == BF else 4
    idx = torch.zeros(8, dtype=torch.int32, device=gpu)
    for r in SR.ROW_REFUSED:
        rows, D, ld, off = r["rows"], r["D"], r["ld"], r["off"]
        if SR.row_check(D, (ld,), (off,), es) == SR.OK:
            continue
        ob, os_, _ = _flat(rows * ld, off, dt, gpu)
        src = torch.zeros(G + rows * ld + 8, dtype=dt, device=gpu)
        tab = torch.zeros(G + rows * ld + 8, dtype=F32, device=gpu)
        sp, tp, op = src.data_ptr() + off * es, tab.data_ptr() + off * 4, os_.data_ptr()
        rcs = [_fn("ug_add_bf16", dt)(sp, ld, sp, ld, op, ld, rows, D, _stream()),
               _fn("ug_add_rowbcast_f32", dt)(op, ld, tp, ld, rows, rows, D, _stream()),
               _fn("ug_gather_rows", dt)(sp, ld, idx.data_ptr(), op, ld, rows, D, _stream()),
               _fn("ug_gate_residual", dt)(None, 0, sp, ld, sp, ld, 1, op, ld, rows, D, _stream())]
        assert rcs == [SR.BAD_ALIGN] * 4, (r, rcs)
        assert bool((_sync_cpu(ob) == SR.SENT).all()), ("a refused call wrote", r)


# ----------------------------------------------------------------------------------------------------------------------------------
# pack / unpack, transpose
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SR.PACK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_pack_unpack_latents(gpu, shape, dt):
    B, Cc, H, W = shape
    assert SR.pack_check(*shape) == SR.OK
    n = B * Cc * H * W
    lat = torch.randn(shape, generator=torch.Generator().manual_seed(n)).to(dt)
    ld, l0 = lat.to(gpu), lat.to(gpu)
    pb, ps, mask = _flat(n, 0, dt, gpu)
    assert _fn("ug_pack_latents", dt)(ld.data_ptr(), ps.data_ptr(), B, Cc, H, W, _stream()) == 0
    want = SR.pack_latents(lat)
    SR.judge_exact(f"pack_latents {shape}", _sync_cpu(pb), _image(want, mask, dt), mask)
    assert torch.equal(ld, l0), "the latents were written"
    ub, us, _ = _flat(n, 0, dt, gpu)
    assert _fn("ug_unpack_latents", dt)(ps.data_ptr(), us.data_ptr(), B, Cc, H, W, _stream()) == 0
    SR.judge_exact(f"unpack_latents {shape}", _sync_cpu(ub), _image(SR.unpack_latents(want, H, W), mask, dt), mask)
    assert torch.equal(us.view(shape), ld), "unpack(pack(x)) != x"
    assert torch.equal(pb.cpu(), _image(want, mask, dt)), "the packed operand was written"


@pytest.mark.parametrize("dt", DTS)
def test_pack_refusals(gpu, dt):
    for shape in SR.PACK_REFUSED:
        assert SR.pack_check(*shape) == SR.BAD_SHAPE
        n = shape[0] * shape[1] * shape[2] * shape[3]
        src = torch.zeros(n + 8, dtype=dt, device=gpu)
        ob, os_, _ = _flat(n, 0, dt, gpu)
        assert _fn("ug_pack_latents", dt)(src.data_ptr(), os_.data_ptr(), *shape, _stream()) == SR.BAD_SHAPE
        assert _fn("ug_unpack_latents", dt)(src.data_ptr(), os_.data_ptr(), *shape, _stream()) == SR.BAD_SHAPE
        assert bool((_sync_cpu(ob) == SR.SENT).all()), ("a refused call wrote", shape)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.TRANSPOSE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_transpose(gpu, c, dt):
    batch, rows, cols, pad, es, ed, eb = c
    ld_s, ld_d = cols + es, pad + ed
    bs_s, bs_d = rows * ld_s + eb, cols * ld_d + eb
    assert SR.transpose_check(rows, cols, pad, ld_s, ld_d) == SR.OK
    g = torch.Generator().manual_seed(rows * 31 + cols)
    src = torch.randn(batch, rows, cols, generator=g).to(dt)
    sfull = torch.zeros(batch * bs_s, dtype=dt)
    dimg = torch.full((G + batch * bs_d + G,), SR.SENT, dtype=dt)
    mask = torch.zeros(dimg.shape, dtype=torch.bool)
    want = SR.transpose(src, pad)
    for b in range(batch):
        sfull[b * bs_s:b * bs_s + rows * ld_s].view(rows, ld_s)[:, :cols] = src[b]
        sl = slice(G + b * bs_d, G + b * bs_d + cols * ld_d)
        mask[sl].view(cols, ld_d)[:, :pad] = True
        dimg[sl].view(cols, ld_d)[:, :pad] = want[b]
    sd, dd = sfull.to(gpu), torch.full(dimg.shape, SR.SENT, dtype=dt).to(gpu)
    s0 = sd.clone()
    assert _fn("ug_transpose", dt)(sd.data_ptr(), ld_s, bs_s, dd[G:].data_ptr(), ld_d, bs_d, batch, rows, cols, pad, _stream()) == 0
    SR.judge_exact(f"transpose {c}", _sync_cpu(dd), dimg, mask)
    assert torch.equal(sd, s0), "the source was written"


# ----------------------------------------------------------------------------------------------------------------------------------
# timestep embedding, small linear
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", SR.TS_CASES + SR.TS_GUIDANCE_CASES, ids=_ids(SR.TS_CASES + SR.TS_GUIDANCE_CASES))
def test_timestep_embed(gpu, c, dt):
    B, dim, ldo = c["B"], c["dim"], c["dim"] + c["slack"]
    t = SR.ts_times(c)
    td = t.to(gpu)
    t0 = td.clone()
    ob, ov, mask = _rows(B, dim, ldo, dt, gpu)
    assert _fn("ug_timestep_embed", dt)(td.data_ptr(), ov.data_ptr(), ldo, B, dim, _stream()) == 0
    truth, a = SR.timestep_embed64(t, dim)
    w = SR.judge_bounded(f"timestep_embed {c['id']}", _sync_cpu(ob), truth, SR.timestep_bound(a, truth, dt), mask)
    if dt == F32:
        got = ob.cpu()[mask].to(F64)
        ck = float(((got - truth.reshape(-1)).abs() / (SR.EPS32 * a.reshape(-1).clamp_min(1.0))).max())
        print(f"timestep_embed_f32 {c['id']}: kernel c = {ck:.2f} (torch {SR.TS_C_TORCH}, bound {SR.TS_MARGIN * SR.TS_C_TORCH})")
    else:
        print(f"timestep_embed bf16 {c['id']}: worst |err| / bound = {w['all']:.3f}")
    assert torch.equal(td, t0), "t was written"


@pytest.mark.parametrize("c", SR.LINEAR_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_small_linear_f32(gpu, c):
    M, N, K, ex, ew, eo, bias, res, silu = c
    x, W, b, R = SR.linear_data(c)
    xv, x0, xf = _operand(M, K, K + ex, F32, gpu, x)
    wv, w0, wf = _operand(N, K, K + ew, F32, gpu, W)
    bd = None if b is None else b.to(gpu)
    Rd = None if R is None else R.to(gpu)
    ob, ov, mask = _rows(M, N, N + eo, F32, gpu)
    from unigen_amd import lib as L
    rc = L.load().ug_small_linear_f32(xv.data_ptr(), K + ex, wv.data_ptr(), K + ew, None if bd is None else bd.data_ptr(), None if Rd is None else Rd.data_ptr(),
                                      N, ov.data_ptr(), N + eo, M, N, K, 1 if silu else 0, _stream())
    assert rc == 0
    img = _sync_cpu(ob)
    SR.judge_guards(f"small_linear_f32 {c}", img, mask)
    truth = SR.small_linear64(x, W, b, R, silu)
    worst = SR.judge_rows(f"small_linear_f32 {c}", img[mask].view(M, N).to(F64), truth, SR.LINEAR_MARGIN * SR.LINEAR_ROW_TORCH)
    print(f"small_linear_f32 {c}: worst row {worst:.3e} (torch F.linear {SR.LINEAR_ROW_TORCH:.1e}, bound {SR.LINEAR_MARGIN * SR.LINEAR_ROW_TORCH:.1e})")
    assert torch.equal(xf, x0) and torch.equal(wf, w0), "an operand was written"


# ----------------------------------------------------------------------------------------------------------------------------------
# optimizer
# ----------------------------------------------------------------------------------------------------------------------------------
class _Stream:
    """one stream of one tensor: n elements at element offset `off` of a 16-byte aligned device buffer of sentinels"""

    def __init__(self, n, off, dt, dev, values=None):
        self.buf, self.view, self.mask = _flat(n, off, dt, dev, values)
        self.dt = dt

    def image(self):
        return self.buf.cpu()

    def ptr(self):
        return self.view.data_ptr() if self.view.numel() else self.buf.data_ptr() + (G * self.buf.element_size())


def _optim_setup(case, p0, dev):
    from unigen_amd import lib as L
    from unigen_amd.optim import chunk_list
    ts, table = [], (L.OptimTensor * len(case))()
    for i, t in enumerate(case):
        n, off = t["n"], t["off"]
        s = dict(grad=_Stream(n, off["grad"], BF if t["gbf"] else F32, dev, torch.zeros(n)),
                 param=_Stream(n, off["param"], BF if t["master"] else F32, dev, p0[i]),
                 master=_Stream(n, off["master"], F32, dev, p0[i]) if t["master"] else None,
                 exp_avg=_Stream(n, off["exp_avg"], F32, dev, torch.zeros(n)), exp_avg_sq=_Stream(n, off["exp_avg_sq"], F32, dev, torch.zeros(n)))
        ts.append(s)
        table[i] = L.optim_tensor(grad=s["grad"].ptr(), grad_dtype=L.UG_DT_BF16 if t["gbf"] else L.UG_DT_F32, numel=n, param=s["param"].ptr(),
                                  param_dtype=L.UG_DT_BF16 if t["master"] else L.UG_DT_F32, master=s["master"].ptr() if t["master"] else 0,
                                  exp_avg=s["exp_avg"].ptr(), exp_avg_sq=s["exp_avg_sq"].ptr(), group=t["group"])
    assert L.load().ug_optim_check_table(C.addressof(table), len(case), len(SR.OPT_GROUPS)) == 0, L.load().ug_last_error()
    dtab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    chunks = chunk_list([t["n"] for t in case])
    assert chunks.shape[0] == sum((t["n"] + SR.CHUNK - 1) // SR.CHUNK for t in case)
    return ts, dtab, chunks.to(dev), chunks.shape[0]


@pytest.mark.parametrize("clip", SR.OPT_CLIP)
@pytest.mark.parametrize("mode", SR.OPT_MODES)
def test_adamw_and_clipping(gpu, mode, clip):
    from unigen_amd import lib as L
    lib = L.load()
    case = SR.optim_case(mode)
    p0, grads = SR.optim_data(case, SR.OPT_MODES.index(mode))
    ts, dtab, dchunks, n_chunks = _optim_setup(case, p0, gpu)
    lr, wd, betas, eps = SR.optim_hyper(case)
    ref = SR.AdamWRef64(p0)
    nc, nc_view, nc_mask = _flat(2, 0, F32, gpu)
    ws = torch.empty(lib.ug_grad_sumsq_workspace_bytes(n_chunks), dtype=torch.uint8, device=gpu)
    worst = {}
    for step in (1, 2):
        gs = grads[step - 1]
        for s, g in zip(ts, gs):
            s["grad"].view.copy_(g)
        before = [s["grad"].image() for s in ts]
        g_eff, coef_ptr = [g.to(F64) for g in gs], None
        if clip != "none":
            assert lib.ug_grad_sumsq(dtab.data_ptr(), len(case), dchunks.data_ptr(), n_chunks, SR.OPT_MAX_NORM, nc_view.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _stream()) == 0
            img = _sync_cpu(nc)
            SR.judge_guards("grad_sumsq norm_coef", img, nc_mask)
            norm, coef = img[nc_mask]
            truth = float(torch.cat([g.to(F64) for g in gs]).norm())
            print(f"{mode} step {step}: total norm {float(norm):.6f}, rel. error vs fp64 {abs(float(norm) - truth) / truth:.2e}; coef {float(coef):.6f}")
            assert abs(float(norm) - truth) <= 1e-6 * truth
            assert torch.equal(coef, SR.clip_coef32(norm, SR.OPT_MAX_NORM)) and float(coef) < 1.0
            assert abs(float(coef) - SR.clip_coef64(truth, SR.OPT_MAX_NORM)) <= 2e-6 * float(coef)
            assert all(torch.equal(s["grad"].image(), b) for s, b in zip(ts, before)), "ug_grad_sumsq wrote a grad"
            if clip == "unfused":
                assert lib.ug_grad_scale(dtab.data_ptr(), len(case), dchunks.data_ptr(), n_chunks, nc_view[1:].data_ptr(), _stream()) == 0
                torch.cuda.synchronize()
                for i, (s, g, t) in enumerate(zip(ts, gs, case)):
                    want = SR.grad_scale(g, float(coef))
                    SR.judge_exact(f"grad_scale {mode} tensor {i} (n {t['n']}, h {t['h_grad']})", s["grad"].image(), _image(want, s["grad"].mask, g.dtype),
                                   s["grad"].mask)
                    g_eff[i] = want.to(F64)
                before = [s["grad"].image() for s in ts]
            else:
                coef_ptr = nc_view[1:].data_ptr()
                g_eff = [g * float(coef) for g in g_eff]
        hp = (L.AdamwGroup * len(SR.OPT_GROUPS))()
        for k, gr in enumerate(SR.OPT_GROUPS):
            for name, val in SR.adamw_hparams(gr["lr"], gr["wd"], gr["betas"], gr["eps"], step).items():
                setattr(hp[k], name, val)
        assert lib.ug_adamw_step(dtab.data_ptr(), len(case), dchunks.data_ptr(), n_chunks, C.addressof(hp), len(SR.OPT_GROUPS), coef_ptr, _stream()) == 0
        torch.cuda.synchronize()
        ref.step(g_eff, lr, wd, betas, eps)
        for i, (s, t) in enumerate(zip(ts, case)):
            name = f"adamw {mode}/{clip} step {step} tensor {i} (n {t['n']}, gbf {t['gbf']}, master {t['master']}, h {t['h']})"
            assert torch.equal(s["grad"].image(), before[i]), f"{name}: the grad was written"
            reg = SR.regions(t["n"], t["h"])
            pm = s["master"] if t["master"] else s["param"]
            for what, st, truth, scale in (("p", pm, ref.p[i], ref.scale_p[i]), ("exp_avg", s["exp_avg"], ref.m[i], ref.scale_m[i]),
                                           ("exp_avg_sq", s["exp_avg_sq"], ref.v[i], ref.scale_v[i])):
                w = SR.judge_bounded(f"{name} {what}", st.image(), truth, SR.adamw_bound(scale), st.mask, reg)
                for r, val in w.items():
                    worst[(what, r)] = max(worst.get((what, r), 0.0), val)
            if t["master"]:
                m_img = s["master"].image()
                SR.judge_exact(f"{name} bf16 param = bf16(master)", s["param"].image(), _image(m_img[s["master"].mask].to(BF), s["param"].mask, BF), s["param"].mask)
    k = SR.ADAMW_MARGIN * SR.ADAMW_K_TORCH
    print(f"adamw {mode}/{clip}: worst error in fp32 epsilons of max(|value|, |update|) (torch {SR.ADAMW_K_TORCH}, bound {k}): "
          + ", ".join(f"{a} {r} {v * k:.2f}" for (a, r), v in sorted(worst.items())))
