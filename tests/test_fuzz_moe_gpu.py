"""Sweep of the MoE routing, dispatch and combine kernels (csrc/moe.hip: the three gates, the three capacity rules, dispatch, the two combines and
their fp32 twins) against the float64 references, case tables and judges of tests/moe_ref.py, which tests/test_moe_ref_cpu.py pins to the oracle.

What is asserted (docs/PARITY_TOLERANCES.md, "MoE routing, dispatch and combine sweep"):
  - gates: the choice judge (distinct; nothing chosen more than 2 delta below the K-th largest float64 logit, nothing more than 2 delta above it left
    out; descending up to 2 delta; exact ties to the lower index), delta = 4 c_lin 2^-24 sum |a w|; at most 3 % of a case's decisions inside the band;
    top-k logits within delta; gate probabilities per element within g (2 delta + 2^-21) + 2^-126; the fp32 twins also at rel-L2 1e-5 / every row 1e-4;
    two runs bit-identical;
  - capacity rules: slot, token_of_slot (with its -1 tail) and exp_counts by integer equality with the index-form rules applied to the device's own
    inputs; weights within 2 fp32 ulps, exactly 0 where dropped; l_aux within 1e-5; every kept choice in exactly one slot, no slot >= capacity;
  - dispatch and the combines: bit equality with the step-by-step rounded float64 chain; the fp32 top-k chain within 2^-22 sum |p y| (+ the tail's ulps).
Every output sits in a buffer of sentinels (before, after, and in the [D, ld) columns of a strided output) that must come back untouched; read-only
operands are compared with their clones; refused argument sets return their code and write nothing. Every case runs: nothing is skipped or filtered."""
import math

import pytest
import torch

from tests import moe_ref as M

pytestmark = pytest.mark.gpu
BF, F32, F64, I32, I64 = M.BF, M.F32, M.F64, torch.int32, torch.int64
G = M.GUARD
DTS = [pytest.param(BF, id="bf16"), pytest.param(F32, id="f32")]
PAD = 4096.0          # what a read-only operand holds in its [D, ld) columns: a kernel that read them would miss every bound


def _sent(dt):
    return M.SENT_F if dt.is_floating_point else M.SENT_I


class Out:
    """an output [rows, D] with leading dimension ld inside a device buffer of sentinels"""

    def __init__(self, rows, D, dt, dev, ld=None, init=None):
        self.rows, self.D, self.ld, self.dt = rows, D, ld or D, dt
        self.buf = torch.full((G + rows * self.ld + G,), _sent(dt), dtype=dt, device=dev)
        self.body = self.buf[G:G + rows * self.ld].view(rows, self.ld)
        self.t = self.body[:, :D]
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init.to(dt))

    def view(self, *shape):
        assert self.ld == self.D
        return self.body.view(*shape)

    def cpu(self):
        torch.cuda.synchronize()
        return self.t.cpu()

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().clone()
        b[G:G + self.rows * self.ld].view(self.rows, self.ld)[:, :self.D] = _sent(self.dt)
        return bool((b == _sent(self.dt)).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == _sent(self.dt)).all())


class Operand:
    """a read-only [rows, D] operand with leading dimension ld; `same()` compares the whole buffer with its clone"""

    def __init__(self, values, dev, ld=None, pad=PAD):
        rows, D = values.shape
        full = torch.full((rows, ld or D), pad, dtype=values.dtype)
        full[:, :D] = values
        self.full = full.to(dev)
        self.t = self.full[:, :D]
        self.clone = self.full.clone()

    def same(self):
        return torch.equal(self.full, self.clone)


def _line(*parts):
    print("MOE", *parts)


# ----------------------------------------------------------------------------------------------------------------------------------
# gates
# ----------------------------------------------------------------------------------------------------------------------------------
def _run_gate(ops, gpu, fam, c, dt, x, cc, wg, noise):
    S, D, E, K = c["S"], c["D"], c["E"], c["K"]
    gates, idx = Out(S, E, F32, gpu), Out(K, S, I32, gpu)
    logits = Out(S, E, F32, gpu) if fam == "topk" else None
    if fam == "top1":
        ops.moe_gate_top1(x.t, cc.t, wg.t, gates.view(S, E), idx.view(S))
    elif fam == "top2":
        ops.moe_gate_top2(x.t, cc.t, wg.t, noise.t if noise is not None else None, gates.view(S, E), idx.view(2, S))
    else:
        ops.moe_gate_topk(x.t, cc.t, wg.t, K, gates.view(S, E), logits.view(S, E), idx.view(K, S))
    assert gates.intact() and idx.intact() and (logits is None or logits.intact()), "a gate wrote outside its outputs"
    return gates, idx, logits


GATE_CASES = [pytest.param(c["family"], c, id=c["id"]) for fam in ("top1", "top2", "topk") for c in M.gate_cases(fam)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("fam,c", GATE_CASES)
def test_gate(gpu, fam, c, dt):
    from unigen_amd import ops
    x_h, c_h, wg_h, noise_h = M.gate_data(c, dt)
    ref = M.gate(x_h, c_h, wg_h, c["K"], noise_h, dt, top2=fam == "top2")
    ld = c["D"] + c["ldx"]
    x, cc, wg = Operand(x_h, gpu, ld), Operand(c_h, gpu, ld), Operand(wg_h, gpu)
    noise = Operand(noise_h, gpu) if noise_h is not None else None
    gates, idx, logits = _run_gate(ops, gpu, fam, c, dt, x, cc, wg, noise)
    again = _run_gate(ops, gpu, fam, c, dt, x, cc, wg, noise)
    for a, b in zip((gates, idx, logits), again):
        assert a is None or torch.equal(a.cpu(), b.cpu()), "two runs differ"
    assert x.same() and cc.same() and wg.same() and (noise is None or noise.same()), "a read-only operand changed"
    share = M.ambiguous_share(ref, c["K"], noise_h, top2=fam == "top2")
    f, msg = M.judge_gate(fam, ref, noise_h, gates.cpu(), idx.cpu(), None if logits is None else logits.cpu())
    scale = M.U * ref["absdot"][:, None]
    klin = 0.0
    if logits is not None and bool((scale > 0).any()):
        ok = (scale > 0).expand_as(ref["logits"])
        klin = float(((logits.cpu().double() - ref["logits"]).abs()[ok] / scale.expand_as(ref["logits"])[ok]).max())
    _line("gate", c["id"], str(dt), f"judge {f:.3g} ambiguous {share:.5f} kernel_c_lin {klin:.3f}")
    assert share <= M.AMBIG_CAP
    assert f <= 1, msg
    if dt == F32:
        v = [M.judge_twin_rows(gates.cpu(), ref["gates"], "gates (twin)")]
        if logits is not None:
            v.append(M.judge_twin_rows(logits.cpu(), ref["logits"], "logits (twin)"))
        f2, msg2 = M.worst(*v)
        _line("gate-twin", c["id"], f"{f2:.3g}")
        assert f2 <= 1, msg2


# ----------------------------------------------------------------------------------------------------------------------------------
# capacity rules
# ----------------------------------------------------------------------------------------------------------------------------------
def _capacity(ops, gpu, rule, gates_h, idx_h, logits_h, uniform_h, E, K, Cc, tag):
    """run one capacity rule on the GPU and hold everything it writes to the index-form rule applied to the same inputs"""
    S = gates_h.shape[0]
    gates, idx = Operand(gates_h.to(F32), gpu), Operand(idx_h.to(I32).view(K, S), gpu)
    slot, tos = Out(K, S, I32, gpu), Out(E, Cc, I32, gpu)
    cnt, l_aux = Out(1, E, I64, gpu), Out(1, 1, F32, gpu)
    w = Out(K, S, F32, gpu) if rule != "rts" else None
    ins = [gates, idx]
    if rule == "rts":
        uni = Operand(uniform_h.to(F32), gpu)
        ins.append(uni)
        ops.moe_capacity_rts(gates.t, idx.t.view(S), uni.t, Cc, slot.view(S), tos.view(E, Cc), cnt.view(E), l_aux.view(1))
        ref = M.capacity_rts(idx_h, uniform_h, E, Cc)
    elif rule == "top2":
        ops.moe_capacity_top2(gates.t, idx.t, Cc, slot.view(2, S), tos.view(E, Cc), w.view(2, S), cnt.view(E), l_aux.view(1))
        ref = M.capacity_top2(idx_h, E, Cc)
    else:
        lg = Operand(logits_h.to(F32), gpu)
        ins.append(lg)
        ops.moe_capacity_topk(gates.t, lg.t, idx.t, Cc, slot.view(K, S), tos.view(E, Cc), w.view(K, S), cnt.view(E), l_aux.view(1))
        ref = M.capacity_topk(idx_h, logits_h, E, Cc)
    for o in (slot, tos, cnt, l_aux, w):
        assert o is None or o.intact(), "a capacity rule wrote outside its outputs"
    assert all(i.same() for i in ins), "a read-only operand changed"
    slot_h = slot.cpu().long().view(ref["slot"].shape)
    v = [M.judge_capacity(slot_h, tos.cpu(), cnt.cpu().view(E), ref, Cc)]
    v.append(M.judge_l_aux(float(l_aux.cpu()), M.l_aux_ref(gates_h, idx_h, E, K if rule == "topk" else None)))
    if w is not None:
        v.append(M.judge_weights(w.cpu(), M.weights_ref(gates_h, idx_h.view(K, S), ref["slot"]), ref["slot"]))
    f, msg = M.worst(*v)
    _line("capacity", tag, f"capacity {Cc} dropped {int((ref['slot'] < 0).sum())} judge {f:.3g} (weights {v[-1][0]:.3g}, l_aux {v[1][0]:.3g})")
    assert f <= 1, msg
    return slot, tos, w


CAP_CASES = [pytest.param(c, id=c["id"]) for rule in M.CAP_KINDS for c in M.capacity_cases(rule)]


@pytest.mark.parametrize("c", CAP_CASES)
def test_capacity_hand_built(gpu, c):
    from unigen_amd import ops
    gates, idx, logits, uniform = M.capacity_data(c)
    _capacity(ops, gpu, c["rule"], gates, idx, logits, uniform, c["E"], c["K"], M.capacity_of(c), c["id"])


@pytest.mark.parametrize("cap", M.CAPS)
@pytest.mark.parametrize("fam", ["top1", "top2", "topk"])
def test_capacity_from_the_devices_own_gate(gpu, fam, cap):
    from unigen_amd import ops
    c = next(c for c in M.gate_cases(fam) if c["S"] == 1025 and c["E"] >= 6 and c["K"] < c["E"])
    x_h, c_h, wg_h, noise_h = M.gate_data(c, BF)
    x, cc, wg = Operand(x_h, gpu), Operand(c_h, gpu), Operand(wg_h, gpu)
    noise = Operand(noise_h, gpu) if noise_h is not None else None
    gates, idx, logits = _run_gate(ops, gpu, fam, c, BF, x, cc, wg, noise)
    S, E, K = c["S"], c["E"], c["K"]
    uniform = torch.rand(S, E, generator=torch.Generator().manual_seed(c["seed"]))
    Cc = M.capacity_of(dict(c, cap=cap))
    _capacity(ops, gpu, {"top1": "rts"}.get(fam, fam), gates.cpu(), idx.cpu().long(), None if logits is None else logits.cpu(), uniform, E, K, Cc,
              f"{c['id']}-cap{cap}")


# ----------------------------------------------------------------------------------------------------------------------------------
# dispatch
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in M.dispatch_cases()])
def test_dispatch(gpu, c, dt):
    from unigen_amd import ops
    x_h, add_h, mod_h, tos_h, Cc = M.dispatch_data(c, dt)
    E, B, D, N = c["E"], c["B"], c["D"], c["N"]
    want = M.dispatch(x_h, add_h, mod_h, tos_h, N, dt)
    x = Operand(x_h, gpu, D + 8)
    add = Operand(add_h.view(E * Cc, D), gpu) if add_h is not None else None
    mod = Operand(mod_h.permute(1, 0, 2).reshape(B * E, D), gpu, D + 64) if mod_h is not None else None      # [B][E] rows, 64 elements wider than the data
    tos = Operand(tos_h.to(I32), gpu)
    out = Out(E * Cc, D, dt, gpu)
    ops.moe_dispatch_modulate(x.t, add.t.view(E, Cc, D) if add else None, mod.t if mod else None, tos.t, out.view(E, Cc, D), E=E, capacity=Cc,
                              tokens_per_sample=N, mod_estride=D + 64, mod_bstride=E * (D + 64))
    assert out.intact(), "dispatch wrote outside its output"
    assert x.same() and tos.same() and (add is None or add.same()) and (mod is None or mod.same())
    got = out.cpu().view(E, Cc, D)
    f, msg = M.judge_equal(got, want, "dispatch")
    empty = bool((got[tos_h < 0] == 0).all())
    _line("dispatch", c["id"], str(dt), f"judge {f:.3g} empty slots {int((tos_h < 0).sum())} zero {empty}")
    assert f == 0 and empty, msg


# ----------------------------------------------------------------------------------------------------------------------------------
# combines
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in M.combine_cases()])
def test_combine(gpu, c, dt):
    from unigen_amd import ops
    d = M.combine_data(c, dt)
    want, bound = M.combine_ref(c, d, dt)
    S, D, E, Cc, N, K, opt = d["S"], c["D"], c["E"], d["C"], c["N"], c["K"], c["opt"]
    yh, yc = Operand(d["yh"].view(E * Cc, D), gpu), Operand(d["yc"].view(E * Cc, D), gpu)
    sbuf = Operand(d["sbuf"].view(6 * N, D), gpu, D + 16)
    out = Out(S, D, dt, gpu, ld=D + 8, init=d["prev"] if opt == "accum" else None)
    kw = dict(E=E, capacity=Cc, accumulate=opt == "accum")
    if opt == "resid":
        kw.update(xs=sbuf.t[:S], cs=sbuf.t[S:2 * S])
    elif opt == "mapped":                                               # the two halves of one [3][2N] buffer
        kw.update(xs=sbuf.t, cs=sbuf.t[N:], s_map=ops.RowMap(N, 2 * N))
    ins = [yh, yc, sbuf]
    if K == 0:
        gates, idx, slot = Operand(d["gates"], gpu), Operand(d["idx"].to(I32)[None], gpu), Operand(d["slot"].to(I32)[None], gpu)
        ins += [gates, idx, slot]
        ops.moe_combine(yh.t.view(E, Cc, D), yc.t.view(E, Cc, D), gates.t, idx.t.view(S), slot.t.view(S), out.t, **kw)
    else:
        ks = S + c["kpad"]                                              # kstride > S: column slices of longer arrays
        w, idx, slot = Operand(d["weights"], gpu, ks, pad=0.75), Operand(d["idx"].to(I32), gpu, ks, pad=1), Operand(d["slot"].to(I32), gpu, ks, pad=1)
        ins += [w, idx, slot]
        ops.moe_combine_topk(yh.t.view(E, Cc, D), yc.t.view(E, Cc, D), w.t, idx.t, slot.t, out.t, **kw)
    assert out.intact(), "combine wrote outside its output"
    assert all(i.same() for i in ins), "a read-only operand changed"
    f, msg = M.judge_bound(out.cpu(), want, bound, "combine")
    exact = float(bound.max()) == 0
    _line("combine", c["id"], str(dt), f"judge {f:.3g} ({'bit equality' if exact else 'fp32 chain bound'}; differing elements {int((out.cpu().double() != want).sum())})")
    assert f <= 1, msg


# ----------------------------------------------------------------------------------------------------------------------------------
# refused argument sets: the documented code, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from unigen_amd import lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    S, D, E, K, Cc = 8, 16, 4, 2, 4
    seen = []
    for dt in (BF, F32):
        sfx = "" if dt == BF else "_f32"
        esz = 2 if dt == BF else 4
        act = lambda *shape: torch.ones(*shape, dtype=dt, device=gpu)
        x, cc, wg, noise = act(S, D + 8), act(S, D + 8), act(32, D), torch.zeros(S, 32, device=gpu)
        gates_in, logits_in = torch.full((S, 32), 1 / 32, device=gpu), torch.zeros(S, 32, device=gpu)
        idx_in = (torch.arange(K * S, device=gpu, dtype=I32) % E).view(K, S).contiguous()
        idx_k = (torch.arange(32, device=gpu, dtype=I32)[:, None] % E).expand(32, S).contiguous()
        slot_in, tos_in, w_in = torch.zeros(32, S, dtype=I32, device=gpu), torch.zeros(E, Cc, dtype=I32, device=gpu), torch.ones(32, S, device=gpu)
        uni = torch.rand(S, 32, device=gpu)
        y, sres, mod = act(E * Cc, D), act(S, D + 8), act(E, D)
        outs = dict(gates=Out(S, 32, F32, gpu), logits=Out(S, 32, F32, gpu), idx=Out(32, S, I32, gpu), slot=Out(32, S, I32, gpu), tos=Out(32, 64, I32, gpu),
                    w=Out(32, S, F32, gpu), cnt=Out(1, 32, I64, gpu), l_aux=Out(1, 1, F32, gpu), disp=Out(E * Cc, D, dt, gpu), comb=Out(S, D + 8, dt, gpu))
        p = lambda t: t.data_ptr()
        o = {k: p(v.t) for k, v in outs.items()}

        def gate(fam, ld=D, S_=S, D_=D, E_=E, K_=K, xoff=0):
            if fam == "top1":
                return getattr(lib, "ug_moe_gate_top1" + sfx)(p(x) + xoff, p(cc), ld, p(wg), S_, D_, E_, o["gates"], o["idx"], st)
            if fam == "top2":
                return getattr(lib, "ug_moe_gate_top2" + sfx)(p(x) + xoff, p(cc), ld, p(wg), S_, D_, E_, p(noise), o["gates"], o["idx"], st)
            return getattr(lib, "ug_moe_gate_topk" + sfx)(p(x) + xoff, p(cc), ld, p(wg), S_, D_, E_, K_, o["gates"], o["logits"], o["idx"], st)

        def capacity(rule, E_=E, K_=K, C_=Cc):
            if rule == "rts":
                return lib.ug_moe_capacity_rts(p(gates_in), p(idx_in), p(uni), S, E_, C_, o["slot"], o["tos"], o["cnt"], o["l_aux"], st)
            if rule == "top2":
                return lib.ug_moe_capacity_top2(p(gates_in), p(idx_in), S, E_, C_, o["slot"], o["tos"], o["w"], o["cnt"], o["l_aux"], st)
            return lib.ug_moe_capacity_topk(p(gates_in), p(logits_in), p(idx_k), S, E_, K_, C_, o["slot"], o["tos"], o["w"], o["cnt"], o["l_aux"], st)

        def dispatch(ldx=D + 8, D_=D, C_=Cc, ooff=0):
            return getattr(lib, "ug_moe_dispatch_modulate" + sfx)(p(x), ldx, None, p(mod), 0, 0, p(tos_in), E, C_, S, D_, o["disp"] + ooff, st)

        def combine(topk, K_=K, ks=S, C_=Cc, xs=True, cs=True, ld_s=D + 8, rpb=0, bstride=0, ldo=D + 8, D_=D, yoff=0):
            tail = (E, C_, p(sres) if xs else None, p(sres) if cs else None, ld_s, rpb, bstride, o["comb"], ldo, S, D_, 0, st)
            if topk:
                return getattr(lib, "ug_moe_combine_topk" + sfx)(p(y) + yoff, p(y), p(w_in), p(idx_k), p(slot_in), K_, ks, *tail)
            return getattr(lib, "ug_moe_combine" + sfx)(p(y) + yoff, p(y), p(gates_in), p(idx_in), p(slot_in), *tail)

        SHAPE, ALIGN, UNSUP = L.UG_ERR_BAD_SHAPE, L.UG_ERR_BAD_ALIGN, L.UG_ERR_UNSUPPORTED
        table = [("E = 17", lambda: gate("top1", E_=17), UNSUP), ("E = 17", lambda: gate("top2", E_=17), UNSUP), ("E = 17", lambda: gate("topk", E_=17), UNSUP),
                 ("E = 1 for top-2", lambda: gate("top2", E_=1), UNSUP), ("K = 0", lambda: gate("topk", K_=0), UNSUP), ("K > E", lambda: gate("topk", K_=E + 1), UNSUP),
                 ("D = 12", lambda: gate("top1", D_=12), ALIGN), ("D = 12", lambda: gate("top2", D_=12), ALIGN), ("D = 12", lambda: gate("topk", D_=12), ALIGN),
                 ("ld = D + 4", lambda: gate("top1", ld=D + 4), ALIGN), ("ld = D + 4", lambda: gate("top2", ld=D + 4), ALIGN),
                 ("ld = D + 4", lambda: gate("topk", ld=D + 4), ALIGN),
                 ("base 8 bytes off", lambda: gate("top1", xoff=8), ALIGN), ("base 8 bytes off", lambda: gate("top2", xoff=8), ALIGN),
                 ("base 8 bytes off", lambda: gate("topk", xoff=8), ALIGN),
                 ("D = 12", lambda: dispatch(D_=12), ALIGN), ("ld = D + 4", lambda: dispatch(ldx=D + 4), ALIGN), ("base 8 bytes off", lambda: dispatch(ooff=8), ALIGN),
                 ("capacity = 0", lambda: dispatch(C_=0), SHAPE)]
        for topk in (False, True):
            table += [("D = 12", lambda t=topk: combine(t, D_=12), ALIGN), ("ld = D + 4", lambda t=topk: combine(t, ldo=D + 4), ALIGN),
                      ("ld = D + 4", lambda t=topk: combine(t, ld_s=D + 4), ALIGN), ("base 8 bytes off", lambda t=topk: combine(t, yoff=8), ALIGN),
                      ("capacity = 0", lambda t=topk: combine(t, C_=0), SHAPE), ("xs without cs", lambda t=topk: combine(t, cs=False), SHAPE),
                      ("cs without xs", lambda t=topk: combine(t, xs=False), SHAPE), ("negative row-map field", lambda t=topk: combine(t, rpb=-1), SHAPE),
                      ("negative row-map field", lambda t=topk: combine(t, rpb=4, bstride=-8), SHAPE)]
        table += [("K = 0", lambda: combine(True, K_=0), SHAPE), ("K = 17", lambda: combine(True, K_=17), SHAPE), ("kstride < S", lambda: combine(True, ks=S - 1), SHAPE)]
        if dt == BF:                                                    # the capacity rules have no twins
            table += [("E = 17", lambda: capacity("rts", E_=17), SHAPE), ("E = 17", lambda: capacity("top2", E_=17), SHAPE),
                      ("E = 17", lambda: capacity("topk", E_=17), SHAPE), ("E = 1 for top-2", lambda: capacity("top2", E_=1), SHAPE),
                      ("K = 0", lambda: capacity("topk", K_=0), SHAPE), ("K > E", lambda: capacity("topk", K_=E + 1), SHAPE),
                      ("capacity = 0", lambda: capacity("rts", C_=0), SHAPE), ("capacity = 0", lambda: capacity("top2", C_=0), SHAPE),
                      ("capacity = 0", lambda: capacity("topk", C_=0), SHAPE)]
        for n, (name, call, code) in enumerate(table):
            rc = call()
            seen.append((str(dt), name, rc))
            assert rc == code, f"{name} (entry {n}, {dt}): returned {rc}, documented {code}"
            assert all(v.untouched() for v in outs.values()), f"{name} (entry {n}, {dt}): refused, but an output was written"
        # the same helpers with nothing wrong are accepted: the refusals above are due to the one argument changed
        for call in (lambda: gate("top1"), lambda: gate("top2"), lambda: gate("topk"), lambda: dispatch(), lambda: combine(False), lambda: combine(True)) + \
                ((lambda: capacity("rts"), lambda: capacity("top2"), lambda: capacity("topk")) if dt == BF else ()):
            assert call() == L.UG_OK
        torch.cuda.synchronize()
    _line("refusals", len(seen), "argument sets refused with their documented code, outputs untouched")
