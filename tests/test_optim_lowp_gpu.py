"""AdamW without fp32 masters / with bf16 moments on the GPU (unigen_amd/optim.py, csrc/optim.hip: ug_adamw_step_lowp, ug_sr_round_bf16) against the
host restatement of tests/optim_lowp_ref.py, bit for bit: the rounding primitive, three steps of every arrangement, independence of the draws
from what else is in the launch, the statistics and the sub-ulp drift with the bounds of tests/test_optim_lowp_ref_cpu.py, state_dict round
trips and conversions, and the tiny FLUX model trained through objective.train_step with a master-less optimizer."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import optim_lowp_ref as R
from tests import test_optim_lowp_ref_cpu as S

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SIZES = [1, 7, 8, 9, 4095, 65535, 65536, 65537, 2 * 65536 + 13]
ARRANGEMENTS = [(False, BF), (False, F32), (True, BF)]
KIND = {(False, BF): (False, "bf16"), (False, F32): (False, "f32"), (True, BF): (True, "bf16"), (True, F32): "master"}
BETAS, EPS = (0.9, 0.999), 1e-8


def _bits(t: torch.Tensor) -> np.ndarray:
    """a tensor's values for a bitwise comparison: uint16 bf16 bits, or fp32"""
    t = t.detach().flatten()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == BF else t.cpu().numpy()


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()          # the bits: NaN equals NaN, 0.0 differs from -0.0


def _views(gpu, sizes, dtype, seed, scale=0.02):
    """tensors of these sizes as views at odd element offsets into one buffer (none of them 16-byte aligned but by accident)"""
    g = torch.Generator().manual_seed(seed)
    offs, at = [], 1
    for n in sizes:
        offs.append(at)
        at += n + (2 if (at + n) % 2 else 1)                # the next offset is odd again
    buf = (scale * torch.randn(at + 8, generator=g)).to(dtype).to(gpu)
    assert all(o % 2 == 1 for o in offs)
    return [buf[o:o + n] for o, n in zip(offs, sizes)]


def _params(gpu, sizes=SIZES, seed=0):
    ps = []
    for v in _views(gpu, sizes, BF, seed):
        p = torch.nn.Parameter(torch.empty(0, device=gpu, dtype=BF))
        p.data = v
        ps.append(p)
    return ps


def _grads(gpu, sizes, dtype, seed):
    return _views(gpu, sizes, dtype, 1000 + seed, scale=1.0)


# ---- 1. the rounding primitive ---------------------------------------------------------------------------------------------------------------
SPECIAL = [0x00000000, 0x80000000, 0x00000001, 0x0000FFFF, 0x80004000, 0x007FFFFF, 0x7F7FFFFF, 0xFF7F8000, 0x7F7F0000, 0x7F800000, 0xFF800000,
           0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x3F800000, 0x3F808000]


def _sr(gpu, x: torch.Tensor, out: torch.Tensor, first, seed, pi, step, word):
    from unigen_amd import lib
    lib.check(lib.load().ug_sr_round_bf16(x.data_ptr(), out.data_ptr(), x.numel(), first, seed, pi, step, word,
                                          torch.cuda.current_stream(gpu).cuda_stream), "ug_sr_round_bf16")


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1023, 65537])
def test_sr_round_matches_the_reference_bitwise(gpu, n):
    g = torch.Generator().manual_seed(n)
    host = torch.randn(n, generator=g)
    hx = host.numpy()                                               # shares host's memory
    hx.view(np.uint32)[:min(n, len(SPECIAL))] = np.array(SPECIAL, dtype=np.uint32)[:min(n, len(SPECIAL))]
    seed = 0xFEDCBA9876543210
    case = 0
    for first in (0, 12345, (1 << 33) + 1):                         # even, odd, and past 2^32 (the counter's second word)
        for ox, oo in [(0, 0), (1, 1), (3, 5), (7, 2), (4, 4), (2, 6), (5, 7), (6, 3)]:
            word, pi, step = case % 3, 5 + case, 1 + case % 4
            case += 1
            xb = torch.zeros(n + 16, dtype=F32, device=gpu)
            ob = torch.full((n + 24,), -7.0, dtype=BF, device=gpu)           # guard values around the output
            x, out = xb[ox:ox + n], ob[8 + oo:8 + oo + n]
            x.copy_(host)
            _sr(gpu, x, out, first, seed, pi, step, word)
            want = R.sr_round(hx, R.draws(seed, pi, step, first + np.arange(n, dtype=np.int64), word))
            got = _bits(ob)
            assert np.array_equal(got[8 + oo:8 + oo + n], want), (n, first, ox, oo, word)
            assert (got[:8 + oo] == 0xC0E0).all() and (got[8 + oo + n:] == 0xC0E0).all(), (n, first, ox, oo)      # nothing written outside


# ---- 2. the step against the reference, bit for bit ---------------------------------------------------------------------------------------
GROUPS = [dict(lr=1e-3, weight_decay=1e-2, seed=0x1234567800000007), dict(lr=3e-4, weight_decay=0.0, seed=99)]
SPLIT = 5                                  # params [0, SPLIT) and the fp32 param: group 0; the rest: group 1, which starts from step count 5
LATER = 5


def _f32_param(gpu):
    p = torch.nn.Parameter(torch.empty(0, device=gpu, dtype=F32))
    p.data = (0.02 * torch.randn(70003, generator=torch.Generator().manual_seed(77))).to(gpu)[3:]
    return p


def _optimizer(gpu, master, sdt, max_grad_norm, seeds=True):
    from unigen_amd.optim import AdamW
    ps, pf = _params(gpu), _f32_param(gpu)
    order = ps[:SPLIT] + [pf] + ps[SPLIT:]                          # param_groups order: the fp32 param has ordinal SPLIT
    groups = [dict(params=ps[:SPLIT] + [pf], **GROUPS[0]), dict(params=ps[SPLIT:], **GROUPS[1])]
    if not seeds:
        groups = [{k: v for k, v in g.items() if k != "seed"} for g in groups]
    opt = AdamW(groups, betas=BETAS, eps=EPS, max_grad_norm=max_grad_norm, master_weights=master, state_dtype=sdt)
    for p in ps[SPLIT:]:
        AdamW._init_state(p, opt.state[p], master, sdt)
        opt.state[p]["step"].fill_(float(LATER))
    return opt, order


def _reference(order, master, sdt):
    ts = []
    for i, p in enumerate(order):
        g = GROUPS[0] if i <= SPLIT else GROUPS[1]
        ts.append(R.Tensor("f32" if p.dtype == F32 else KIND[(master, sdt)], _bits(p), param_index=i, seed=g["seed"], step=0 if i <= SPLIT else LATER))
    return ts


def _coef(opt, max_grad_norm):
    """the fused clip coefficient of the step just taken, from its norm: csrc/optim.hip sumsq_final_kernel's fp32 operations"""
    norm = np.float32(opt.last_grad_norm.item())
    c = (np.float32(1.0) / (norm + np.float32(1e-6))) * np.float32(max_grad_norm)
    return np.float32(1.0) if c > np.float32(1.0) else c


@pytest.mark.parametrize("max_grad_norm", [None, 1.0], ids=["noclip", "clip"])
@pytest.mark.parametrize("master,sdt", ARRANGEMENTS, ids=["nomaster-bf16", "nomaster-f32", "master-bf16"])
def test_step_matches_the_reference_bitwise(gpu, master, sdt, max_grad_norm):
    opt, order = _optimizer(gpu, master, sdt, max_grad_norm)
    dflt, dorder = _optimizer(gpu, True, F32, max_grad_norm, seeds=False)       # the default optimizer on the same params and grads
    ref = _reference(order, master, sdt)
    sizes = [p.numel() for p in order]
    for s in range(3):
        gb = _grads(gpu, sizes, BF, s)
        for p, q, g in zip(order, dorder, gb):
            p.grad = g if p.dtype == BF else g.float()
            q.grad = p.grad
        opt.step(); dflt.step()
        coef = None
        if max_grad_norm is not None:
            assert torch.equal(opt.last_grad_norm, dflt.last_grad_norm) and float(opt.last_grad_norm) > max_grad_norm
            coef = _coef(opt, max_grad_norm)
        for i, (t, p) in enumerate(zip(ref, order)):
            h = GROUPS[0] if i <= SPLIT else GROUPS[1]
            t.update(R.widen(_bits(p.grad)) if p.grad.dtype == BF else _bits(p.grad), h["lr"], BETAS, EPS, h["weight_decay"], coef)
            st = opt.state[p]
            assert int(st["step"]) == t.step
            assert _same(_bits(p), t.p), (s, i, "param")
            assert _same(_bits(st["exp_avg"]), t.m), (s, i, "exp_avg")
            assert _same(_bits(st["exp_avg_sq"]), t.v), (s, i, "exp_avg_sq")
            assert ("master_param" in st) == (t.master is not None)
            if t.master is not None:
                assert _same(_bits(st["master_param"]), t.master), (s, i, "master")
    # the fp32 param in the low-precision launch: the default optimizer's bits; bf16 params do differ from the default's
    pf, qf = order[SPLIT], dorder[SPLIT]
    assert pf.dtype == F32 and torch.equal(pf, qf) and torch.equal(opt.state[pf]["exp_avg_sq"], dflt.state[qf]["exp_avg_sq"])
    assert opt.state[pf]["exp_avg"].dtype == F32 and "master_param" not in opt.state[pf]
    if not master:
        assert not torch.equal(order[-1], dorder[-1])


def _raw_case(gpu, master, sdt, grad_dtype, use_coef, n, seed):
    """one tensor through the C entry point: how fp32 grads reach a bf16 param (torch refuses such a .grad)"""
    from unigen_amd import lib
    from unigen_amd.optim import _upload, chunk_list
    p = _views(gpu, [n], BF, seed)[0]
    g = _views(gpu, [n], grad_dtype, seed + 1, scale=1.0)[0]
    m, v = (_views(gpu, [n], sdt, seed + k, scale=s)[0] for k, s in ((2, 0.1), (3, 0.01)))
    v.abs_()
    mst = _views(gpu, [n], F32, seed + 4)[0] if master else None
    ref = R.Tensor(KIND[(master, sdt)], _bits(p), param_index=3, seed=17, step=6)
    ref.m, ref.v = _bits(m).copy(), _bits(v).copy()
    if master:
        ref.master = _bits(mst).copy()
    table = (lib.OptimTensorLP * 1)()
    d = table[0]
    d.param, d.grad, d.master, d.exp_avg, d.exp_avg_sq, d.numel = p.data_ptr(), g.data_ptr(), mst.data_ptr() if master else None, m.data_ptr(), v.data_ptr(), n
    d.param_dtype, d.grad_dtype, d.state_dtype = lib.UG_DT_BF16, lib.UG_DT_BF16 if grad_dtype == BF else lib.UG_DT_F32, lib.UG_DT_BF16 if sdt == BF else lib.UG_DT_F32
    d.group, d.param_index = 0, 3
    cdll = lib.load()
    lib.check(cdll.ug_optim_check_table_lowp(C.addressof(table), 1, 1), "ug_optim_check_table_lowp")
    dtab = _upload(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8), gpu)
    chunks = chunk_list([n])
    dch = _upload(chunks, gpu)
    hp = (lib.AdamwGroupLP * 1)()
    coef = torch.tensor([0.37], dtype=F32, device=gpu) if use_coef else None
    for step in (7, 8, 9):
        for k, val in R.hyper(1e-3, BETAS, EPS, 1e-2, step).items():
            setattr(hp[0], k, float(val))
        hp[0].step, hp[0].seed = step, 17
        g.copy_(_views(gpu, [n], grad_dtype, seed + step, scale=1.0)[0])
        gbits = _bits(g)
        gref = R.widen(gbits) if grad_dtype == BF else gbits
        lib.check(cdll.ug_adamw_step_lowp(dtab.data_ptr(), 1, dch.data_ptr(), chunks.shape[0], C.addressof(hp), 1, coef.data_ptr() if use_coef else None,
                                          torch.cuda.current_stream(gpu).cuda_stream), "ug_adamw_step_lowp")
        ref.update(gref, 1e-3, BETAS, EPS, 1e-2, np.float32(0.37) if use_coef else None)
        assert ref.step == step
        assert _same(_bits(p), ref.p) and _same(_bits(m), ref.m) and _same(_bits(v), ref.v), (master, sdt, grad_dtype, use_coef, n, step)
        if master:
            assert _same(_bits(mst), ref.master)
        assert _same(_bits(g), gbits)                                                # grads are only read


@pytest.mark.parametrize("grad_dtype", [F32, BF], ids=["gf32", "gbf16"])
@pytest.mark.parametrize("master,sdt", ARRANGEMENTS, ids=["nomaster-bf16", "nomaster-f32", "master-bf16"])
def test_raw_step_with_either_grad_dtype_from_running_state(gpu, master, sdt, grad_dtype):
    """three steps of the C entry point from a state in mid-run (non-zero moments of the state dtype, step count 6), fp32 and bf16 grads, with and
    without the clip coefficient: how fp32 grads reach a bf16 param at all"""
    for i, n in enumerate(SIZES):
        _raw_case(gpu, master, sdt, grad_dtype, use_coef=bool(i % 2), n=n, seed=10 * i)


# ---- 3. composition does not matter ---------------------------------------------------------------------------------------------------------
def test_draws_do_not_depend_on_what_else_is_in_the_launch(gpu):
    from unigen_amd.optim import AdamW
    sizes = [7, 4095, 65537, 9, 65536 + 13]

    def run(seed=3, skip=((), ()), realloc=False):
        ps = _params(gpu, sizes, seed=4)
        opt = AdamW(ps, lr=1e-3, master_weights=False, state_dtype=BF, seed=seed)
        for s in range(2):
            gs = _grads(gpu, sizes, BF, s)
            if realloc:                                             # every grad at another address and alignment than the run compared to
                gs = [torch.cat([g.new_zeros(4), g])[4:] for g in gs]
            for i, (p, g) in enumerate(zip(ps, gs)):
                p.grad = None if i in skip[s] else g
            opt.step()
            opt.zero_grad(set_to_none=True)
        return ps, opt

    full, fo = run()
    # some grads None at the second step: the other params get the bits of the all-grads run, the skipped ones keep their step-1 bits and count
    part, po = run(skip=((), (1, 3)))
    for i in (0, 2, 4):
        assert torch.equal(full[i], part[i]) and torch.equal(fo.state[full[i]]["exp_avg_sq"], po.state[part[i]]["exp_avg_sq"])
    assert all(int(po.state[part[i]]["step"]) == 1 and not torch.equal(full[i], part[i]) for i in (1, 3))
    # a param that joins only at the second step (its first): no state before, its ordinal unchanged
    late, lo = run(skip=((0, 2), ()))
    for i in (1, 3, 4):
        assert torch.equal(full[i], late[i])
    assert int(lo.state[late[0]]["step"]) == 1
    # zero_grad(set_to_none=True) and new grad tensors elsewhere: the same bits
    moved, mo = run(realloc=True)
    assert all(torch.equal(a, b) for a, b in zip(full, moved))
    assert all(torch.equal(fo.state[a]["exp_avg"], mo.state[b]["exp_avg"]) for a, b in zip(full, moved))
    # another seed: other bits
    other, _ = run(seed=4)
    assert all(not torch.equal(full[i], other[i]) for i in (1, 2, 4))            # the tensors of thousands of elements
    # another step or param ordinal: other draws for the same values
    x = torch.randn(4096, device=gpu)
    outs = []
    for pi, step in ((0, 1), (0, 2), (1, 1)):
        o = torch.empty(4096, dtype=BF, device=gpu)
        _sr(gpu, x, o, 0, 3, pi, step, 0)
        outs.append(o)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---- 4. statistics and drift, with the bounds of the host tests -------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
def test_kernel_statistics(gpu, step):
    n, seed, pi = S.STAT_N, 12345, 3
    e = np.arange(n, dtype=np.int64)
    out = torch.empty(n, dtype=BF, device=gpu)
    for f in S.STAT_FRACTIONS:
        x = torch.full((n,), float(S.stat_value(f)), dtype=F32, device=gpu)
        _sr(gpu, x, out, 0, seed, pi, step, 0)
        got = _bits(out)
        dev, bound = S.mean_within_bound(got, f)
        print(f"step {step} f {f}: mean of the kernel's rounded values {dev:.2f} sigma from the value (bound {bound})")
        assert dev <= bound
        assert np.array_equal(got, R.sr_round(np.full(n, S.stat_value(f)), R.draws(seed, pi, step, e, 0)))
    # the bucket (top 4 bits) of each draw, read off the kernel: 1 + k / 16 ulp rounds up exactly when the bucket is >= 16 - k
    for word in range(3):
        bucket = np.zeros(n, dtype=np.int64)
        for k in range(1, 16):
            x = torch.full((n,), 1.0 + 2.0 ** -7 * k / 16, dtype=F32, device=gpu)
            _sr(gpu, x, out, 0, seed, pi, step, word)
            bucket += _bits(out) == 0x3F81
        c = S.chi2_16(bucket << 12)
        print(f"step {step} word {word}: chi-square of the kernel's draws over 16 buckets {c:.1f} (bound {S.CHI2_16_BUCKETS_0999})")
        assert c < S.CHI2_16_BUCKETS_0999
        assert np.array_equal(bucket, (R.draws(seed, pi, step, e, word) >> 12).astype(np.int64))


def test_sub_ulp_updates_drift_as_the_masters_do(gpu):
    """65536 weights at 1.0, a constant gradient of -1, lr = 2^-11 (1/16 bf16 ulp), no weight decay: AdamW's update is lr to within fp32 rounding
    (1e-6 of it), so 64 steps move an exact weight by 4 ulp. The master-less param (fp32 moments: the update itself is exact) follows in the mean,
    to the host test's bound; the default optimizer's master moves by 4 ulp; rounding each update to nearest would never leave 1.0."""
    from unigen_amd.optim import AdamW
    n, ulp = S.DRIFT_N, 2.0 ** -7
    make = lambda: torch.nn.Parameter(torch.ones(n, dtype=BF, device=gpu))
    p_sr, p_m = make(), make()
    o_sr = AdamW([p_sr], lr=ulp * S.DRIFT_ULPS, betas=BETAS, eps=EPS, weight_decay=0.0, master_weights=False, state_dtype=F32, seed=9)
    o_m = AdamW([p_m], lr=ulp * S.DRIFT_ULPS, betas=BETAS, eps=EPS, weight_decay=0.0)
    g = torch.full((n,), -1.0, dtype=BF, device=gpu)
    for _ in range(S.DRIFT_STEPS):
        p_sr.grad = p_m.grad = g
        o_sr.step(); o_m.step()
    moved = float((p_sr.detach().double() - 1.0).mean()) / ulp
    master = float((o_m.state[p_m]["master_param"].double() - 1.0).mean()) / ulp
    print(f"mean displacement: master-less {moved:.4f} ulp, the default's masters {master:.6f} ulp (bound {S.drift_bound_ulps():.3f} ulp around 4)")
    assert abs(master - S.DRIFT_STEPS * S.DRIFT_ULPS) <= 1e-3
    assert abs(moved - S.DRIFT_STEPS * S.DRIFT_ULPS) <= S.drift_bound_ulps() and abs(moved - master) <= S.drift_bound_ulps()
    assert len(torch.unique(p_sr.detach())) > 1                       # individual weights differ: it is the mean that follows


# ---- 5. state_dict ----------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_conversions(gpu):
    from unigen_amd.optim import AdamW
    sizes = [9, 4095, 65537]
    kw = dict(lr=1e-3, max_grad_norm=1.0, master_weights=False, state_dtype=BF, seed=21)

    def feed(ps, s):
        for p, g in zip(ps, _grads(gpu, sizes, BF, s)):
            p.grad = g

    full = _params(gpu, sizes, seed=6)
    o = AdamW(full, **kw)
    for s in range(4):
        feed(full, s); o.step()
    half = _params(gpu, sizes, seed=6)
    o1 = AdamW(half, **kw)
    for s in range(2):
        feed(half, s); o1.step()
    sd = o1.state_dict()
    assert all(sd["param_groups"][0][k] == v for k, v in dict(master_weights=False, state_dtype=BF, seed=21).items())
    for st, p in zip(sd["state"].values(), half):
        assert "master_param" not in st and st["exp_avg"].dtype == BF and st["exp_avg_sq"].dtype == BF
        assert sum(t.numel() * t.element_size() for t in st.values() if torch.is_tensor(t) and t.is_cuda) == 4 * p.numel()    # 4 B per element
    resumed = [torch.nn.Parameter(p.detach().clone()) for p in half]
    o2 = AdamW(resumed, **kw)
    o2.load_state_dict(sd)
    assert all(o2.state[p]["exp_avg"].dtype == BF and "master_param" not in o2.state[p] and float(o2.state[p]["step"]) == 2 for p in resumed)
    for s in range(2, 4):
        feed(resumed, s); o2.step()
    for x, y in zip(full, resumed):
        assert torch.equal(x, y)                                    # the bits of the uninterrupted run
        assert all(torch.equal(o.state[x][k], o2.state[y][k]) for k in ("exp_avg", "exp_avg_sq"))
    # low-precision state -> a default group: fp32 moments (exact), masters seeded from the params; the group keeps its own options
    d = AdamW([torch.nn.Parameter(p.detach().clone()) for p in half], lr=1e-3)
    d.load_state_dict(sd)
    assert d.param_groups[0]["master_weights"] is True and d.param_groups[0]["state_dtype"] == F32
    for p, q in zip(d.param_groups[0]["params"], half):
        st = d.state[p]
        assert st["exp_avg"].dtype == F32 and torch.equal(st["exp_avg"], o1.state[q]["exp_avg"].float())
        assert torch.equal(st["exp_avg_sq"], o1.state[q]["exp_avg_sq"].float()) and torch.equal(st["master_param"], p.detach().float())
    feed(d.param_groups[0]["params"], 2); d.step()
    assert float(d.state[d.param_groups[0]["params"][0]]["step"]) == 3
    # fp32-master state -> a master-less group: the masters are dropped, the moments rounded to bf16 (nearest) once
    dsd = d.state_dict()
    assert "master_param" in next(iter(dsd["state"].values()))
    back = AdamW([torch.nn.Parameter(p.detach().clone()) for p in d.param_groups[0]["params"]], **kw)
    back.load_state_dict(dsd)
    assert back.param_groups[0]["master_weights"] is False and back.param_groups[0]["state_dtype"] == BF and back.param_groups[0]["seed"] == 21
    for p, q in zip(back.param_groups[0]["params"], d.param_groups[0]["params"]):
        st = back.state[p]
        assert "master_param" not in st and st["exp_avg"].dtype == BF and float(st["step"]) == 3
        assert torch.equal(st["exp_avg"], d.state[q]["exp_avg"].to(BF)) and torch.equal(st["exp_avg_sq"], d.state[q]["exp_avg_sq"].to(BF))
    feed(back.param_groups[0]["params"], 3); back.step()
    assert all("master_param" not in back.state[p] and float(back.state[p]["step"]) == 4 for p in back.param_groups[0]["params"])


# ---- 6. the tiny model through train_step -----------------------------------------------------------------------------------------------------
def test_tiny_model_trains_through_train_step_without_masters(gpu):
    from oracle import unigen_ref as Rf
    from tests.test_training_gpu import CONTROL, TINY, _dev
    from unigen_amd import objective as O
    from unigen_amd.flux import UniGenFlux
    from unigen_amd.optim import AdamW

    def build():
        m = UniGenFlux.from_config(dict(TINY), device=gpu, dtype=BF)
        m.init_condition_block(condition_nums=1, condition_types=["canny"], control_params=dict(CONTROL))
        return m

    model = build()
    model.init_synthetic_(seed=3, std=0.05, bias_std=0.02)
    model.init_trainable_param()
    B, grid, T, Cl = 2, 8, 64, 16
    rcfg = Rf.FluxConfig(condition_nums=1, **TINY)
    inp = Rf.make_inputs(rcfg, B=B, grid=grid, T=T)
    hidden = inp.pop("hidden_states")
    kw = {k: _dev(v, gpu, BF if k != "gate_uniform" and not k.endswith("_ids") else None) for k, v in inp.items()}
    t = torch.full((B,), 0.75, dtype=BF, device=gpu)
    with torch.no_grad():
        model(hidden_states=hidden.to(gpu).to(BF), timestep=t, **kw)        # the packs exist from here on: trainable params may be views into them
    g = torch.Generator().manual_seed(21)
    batch = dict(latents=torch.randn(B, Cl, 2 * grid, 2 * grid, generator=g).to(BF).to(gpu), noise=torch.randn(B, Cl, 2 * grid, 2 * grid, generator=g).to(BF).to(gpu),
                 u=torch.tensor((0.25, 0.731), dtype=F32, device=gpu), **kw)
    names = {n for n, p in model.named_parameters() if p.requires_grad}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    versions = {n: p._version for n, p in model.named_parameters()}
    opt = AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2, master_weights=False, state_dtype=BF, seed=1)
    obj = O.FlowMatchObjective("none")
    losses = [float(O.train_step(model, opt, obj, dict(batch), max_grad_norm=1.0)["step_loss"]) for _ in range(4)]
    print("train_step losses with a master-less optimizer:", [f"{x:.5f}" for x in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    stepped = {n for n, p in model.named_parameters() if p in opt.state and opt.state[p]}
    assert stepped and stepped <= names
    for n, p in model.named_parameters():
        st = opt.state.get(p, {})
        if n not in names:
            assert torch.equal(p.detach(), before[n]), n                 # frozen: bitwise unchanged
        elif n in stepped:
            assert p._version > versions[n], n
            assert "master_param" not in st and st["exp_avg"].dtype == (BF if p.dtype == BF else F32)
    assert sum(not torch.equal(model.get_parameter(n).detach(), before[n]) for n in stepped) >= len(stepped) // 2
    with torch.no_grad():                                                # the inference path reads the updated packed weights
        trained = model(hidden_states=hidden.to(gpu).to(BF), timestep=t, **kw)[0]
        fresh = build()
        fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
        again = fresh(hidden_states=hidden.to(gpu).to(BF), timestep=t, **kw)[0]
    assert torch.equal(trained, again)
