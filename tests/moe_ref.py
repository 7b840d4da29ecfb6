"""Float64 references, case tables and judges for the MoE routing, dispatch and combine kernels (csrc/moe.hip), written from the contract in
include/unigen_hip.h. Plain torch on the CPU; tests/test_moe_ref_cpu.py pins it to the oracle and shows that each plausible slip fails a judge,
tests/test_fuzz_moe_gpu.py holds the kernels to it (docs/PARITY_TOLERANCES.md, "MoE routing, dispatch and combine sweep").

Every judge returns (factor, message): factor <= 1 passes; for a bounded check it is the worst error over its bound, for an integer or bit-equality
check it is inf when anything differs (the message carries the count and the first place)."""
import math
import random

import torch

from oracle import unigen_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24                      # unit roundoff of fp32
EPS32 = float(torch.finfo(F32).eps)
GUARD = 64                          # sentinel elements before and after every output
SENT_F, SENT_I = -12288.0, -7777777  # exactly representable in bf16; no slot, token, expert or count
INF = float("inf")

# max |torch fp32 F.linear - float64| / (2^-24 absdot) over every committed gate case, both dtypes (tests/test_moe_ref_cpu.py re-measures it and
# asserts the re-measurement within [1/2, 1] of this figure). The kernel is allowed KERNEL_MARGIN x this: the step sweep's rule for ug_small_linear_f32.
C_LIN = 12.0
KERNEL_MARGIN = 4.0
AMBIG_CAP = 0.03                    # at most this share of a case's (token, choice) decisions may lie inside the 2 delta band
EXP_SLACK = 2.0 ** -21              # a few fp32 roundings of exp, sum and division


def rnd(t: torch.Tensor, dt) -> torch.Tensor:
    """float64 -> one fp32 operation's result -> the working type -> float64: exactly what a kernel's `EL::rnd(fp32 expression)` keeps."""
    return t.to(F32).to(dt).to(F64)


def _ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max err / bound; 0 / 0 = 0, x / 0 = inf, NaN = inf"""
    if err.numel() == 0:
        return 0.0
    err, bound = err.to(F64), bound.to(F64).expand_as(err)
    r = torch.where(err <= bound, torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)),
                    torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.full_like(err, INF)))
    r = torch.where(torch.isnan(err) | torch.isnan(r), torch.full_like(r, INF), r)
    return float(r.max())


def judge_equal(got: torch.Tensor, want: torch.Tensor, what: str):
    """integer / bit equality (values compared in `got`'s type; NaN never equals)"""
    got, want = got.cpu(), want.cpu()
    if got.shape != want.shape:
        return INF, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = ~(got == want.to(got.dtype))
    n = int(bad.sum())
    if n == 0:
        return 0.0, ""
    at = tuple(int(v) for v in torch.nonzero(bad)[0])
    return INF, f"{what}: {n} of {bad.numel()} differ, first at {at}: got {got[at].item()} want {want[at].item()}"


def judge_bound(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str):
    err = (got.cpu().to(F64) - want.to(F64)).abs()
    f = _ratio(err, bound)
    return f, ("" if f <= 1 else f"{what}: worst error {f:.3g} x its bound")


def worst(*verdicts):
    """the worst of several (factor, message) verdicts"""
    f = max((v[0] for v in verdicts), default=0.0)
    return f, "; ".join(v[1] for v in verdicts if v[1])


# ----------------------------------------------------------------------------------------------------------------------------------
# gate
# ----------------------------------------------------------------------------------------------------------------------------------
def gate(x, c, wg, K, noise=None, dtype=BF, top2=False):
    """operand a = rnd(x + c) (bf16 kernels: the reference's bf16 `hidden + condition`; fp32 twins: the fp32 sum). Returns float64 logits and softmax,
    absdot[s] = max_e sum_d |a_d wg_ed| (the scale of one fp32 logit's error), delta[s] (the kernel's allowed logit error) and the float64 choices
    idx [K][S]: descending logit, the lower expert first among equals; top2: [argmax, argmax of logits + noise over the others]."""
    a = rnd(x.to(F64) + c.to(F64), dtype)
    w = wg.to(F64)
    uniq, inv = torch.unique(w, dim=0, return_inverse=True)          # one evaluation per distinct row: identical rows give identical logits whatever
    logits = (a @ uniq.t())[:, inv]                                   # order the host's BLAS sums a column in, as they do in the kernel
    absdot = (a.abs() @ w.abs().t()).max(1).values
    out = dict(a=a, logits=logits, gates=torch.softmax(logits, 1), absdot=absdot, delta=KERNEL_MARGIN * C_LIN * U * absdot)
    if top2:
        i1 = torch.sort(logits, dim=1, descending=True, stable=True)[1][:, 0]
        v = second_values(logits, noise, i1)
        out["idx"] = torch.stack([i1, torch.sort(v, dim=1, descending=True, stable=True)[1][:, 0]])
        out["delta2"] = out["delta"] + (0.0 if noise is None else U * noise.to(F64).abs().max(1).values)
    else:
        out["idx"] = torch.sort(logits, dim=1, descending=True, stable=True)[1][:, :K].t().contiguous()
    return out


def second_values(logits, noise, first):
    """what top-2's second choice ranks: logits + noise over the experts other than the first choice"""
    v = logits.to(F64) if noise is None else logits.to(F64) + noise.to(F64)
    return v.masked_fill(torch.nn.functional.one_hot(first.long(), logits.shape[1]).bool(), -INF)


def judge_choices(idx, vals, delta, what="choices"):
    """idx [K][S] against float64 vals [S][E] (-inf = not in the competition) whose fp32 evaluation may be off by delta[s]: distinct; every chosen
    value >= the K-th largest - 2 delta; every value > the K-th largest + 2 delta chosen; descending up to 2 delta; among exactly equal values the
    lower index first (decided exactly: the kernel's fp32 sums are bit-identical there)."""
    idx = idx.cpu().long()
    K, S = idx.shape
    E = vals.shape[1]
    if int(idx.min()) < 0 or int(idx.max()) >= E:
        return INF, f"{what}: expert out of range"
    chosen = torch.zeros(S, E, dtype=torch.bool).scatter_(1, idx.t(), True)
    if not bool((chosen.sum(1) == K).all()):
        s = int(torch.nonzero(chosen.sum(1) != K)[0])
        return INF, f"{what}: token {s} chooses {idx[:, s].tolist()}: not distinct"
    cv = vals.gather(1, idx.t())                                  # [S][K]
    if bool(torch.isinf(cv).any()):
        return INF, f"{what}: an excluded expert was chosen"
    kth = torch.topk(vals, K, dim=1).values[:, -1]
    band = (2 * delta).to(F64)
    zero = torch.zeros(())
    f_low = _ratio(torch.maximum(kth[:, None] - cv, zero), band[:, None])
    over = torch.where(chosen, torch.full_like(vals, -INF), vals) - kth[:, None]
    f_miss = _ratio(torch.maximum(over, zero), band[:, None])
    f_ord = _ratio(torch.maximum(cv[:, 1:] - cv[:, :-1], zero), band[:, None]) if K > 1 else 0.0
    pos = torch.full((S, E), K, dtype=torch.long).scatter_(1, idx.t(), torch.arange(K).expand(S, K))
    ties = 0
    for e1 in range(E):
        for e2 in range(e1 + 1, E):
            ties += int(((vals[:, e1] == vals[:, e2]) & torch.isfinite(vals[:, e1]) & (pos[:, e2] < pos[:, e1])).sum())
    f = max(f_low, f_miss, f_ord, INF if ties else 0.0)
    msg = "" if f <= 1 else f"{what}: chosen below the K-th {f_low:.3g}x, clear winner left out {f_miss:.3g}x, order {f_ord:.3g}x the band; {ties} exact ties to the higher index"
    return f, msg


def judge_top2_choices(idx, ref, noise):
    idx = idx.cpu().long()
    v1 = judge_choices(idx[:1], ref["logits"], ref["delta"], "first choice")
    if bool((idx[0] == idx[1]).any()):
        return INF, f"second choice equals the first on {int((idx[0] == idx[1]).sum())} tokens"
    return worst(v1, judge_choices(idx[1:], second_values(ref["logits"], noise, idx[0]), ref["delta2"], "second choice"))


def ambiguous(vals, delta, K):
    """bool [S][K]: decision k of a token lies inside the band if the k-th largest value has a neighbour in the ranking within 2 delta that is not
    exactly equal (exact ties are decided by index)"""
    v = torch.sort(vals, 1, descending=True)[0]
    S, E = v.shape
    gap = v[:, :-1] - v[:, 1:]
    near = torch.nan_to_num(gap, nan=INF) <= (2 * delta)[:, None]
    near &= gap > 0
    near = torch.cat([torch.zeros(S, 1, dtype=torch.bool), near, torch.zeros(S, 1, dtype=torch.bool)], 1)     # near[:, j]: between rank j-1 and j
    return (near[:, :K] | near[:, 1:K + 1])


def ambiguous_share(ref, K, noise=None, top2=False) -> float:
    if top2:
        a = torch.cat([ambiguous(ref["logits"], ref["delta"], 1), ambiguous(second_values(ref["logits"], noise, ref["idx"][0]), ref["delta2"], 1)], 1)
    else:
        a = ambiguous(ref["logits"], ref["delta"], K)
    return float(a.double().mean())


def judge_logits(got, ref):
    return judge_bound(got, ref["logits"], ref["delta"][:, None], "logits")


def judge_gates(got, ref):
    """per element within g64 (2 delta + 2^-21) + 2^-126: both logit errors (the element's and the normaliser's) and the fp32 roundings of exp, sum, division"""
    g = ref["gates"]
    return judge_bound(got, g, g * (2 * ref["delta"][:, None] + EXP_SLACK) + 2.0 ** -126, "gates")


def judge_gate(family, ref, noise, gates, idx, logits=None):
    """everything a gate kernel writes, against its reference: the verdict the GPU test asserts and the mutation study must overturn"""
    idx = idx.cpu().long()
    if family == "top2":
        return worst(judge_gates(gates, ref), judge_top2_choices(idx.view(2, -1), ref, noise))
    v = [judge_gates(gates, ref), judge_choices(idx.view(-1, ref["logits"].shape[0]), ref["logits"], ref["delta"])]
    if family == "topk":
        v.append(judge_logits(logits, ref))
    return worst(*v)


def judge_twin_rows(got, want, what):
    """the fp32 twins' project bound: rel-L2 <= 1e-5 over the tensor and <= 1e-4 on every row"""
    d = got.cpu().to(F64) - want
    f_all = _ratio(d.norm()[None], 1e-5 * want.norm()[None])
    f_row = _ratio(d.norm(dim=1), 1e-4 * want.norm(dim=1))
    f = max(f_all, f_row)
    return f, ("" if f <= 1 else f"{what}: rel-L2 {f_all:.3g} x 1e-5, worst row {f_row:.3g} x 1e-4")


# ----------------------------------------------------------------------------------------------------------------------------------
# capacity rules, index form; inputs are a device's own idx / gates / logits, so every comparison is integer equality
# ----------------------------------------------------------------------------------------------------------------------------------
def _fill(E, capacity, S, K):
    return (torch.full((K, S), -1, dtype=torch.long), torch.full((E, capacity), -1, dtype=torch.long), torch.zeros(E, dtype=torch.long))


def capacity_rts(idx, uniform, E, capacity):
    """top-1 with Random Token Selection: an expert keeps the `capacity` largest draws among its tokens, the earlier token among equal draws; slots
    in token order; counts before the drop"""
    idx = idx.cpu().long().view(-1)
    S = idx.numel()
    slot, tos, cnt = _fill(E, capacity, S, 1)
    for e in range(E):
        toks = torch.nonzero(idx == e).flatten()
        cnt[e] = toks.numel()
        if toks.numel() > capacity:
            order = torch.sort(uniform.cpu()[toks, e].to(F64), descending=True, stable=True)[1]
            toks = toks[torch.sort(order[:capacity])[0]]
        slot[0, toks] = torch.arange(toks.numel())
        tos[e, :toks.numel()] = toks
    return dict(slot=slot[0], tos=tos, counts=cnt)


def capacity_top2(idx, E, capacity):
    """top-2: first choices take slots in token order, second choices queue behind ALL first choices of the expert"""
    idx = idx.cpu().long()
    S = idx.shape[1]
    slot, tos, cnt = _fill(E, capacity, S, 2)
    for e in range(E):
        fill = 0
        for k in range(2):
            toks = torch.nonzero(idx[k] == e).flatten()
            loc = fill + torch.arange(toks.numel())
            keep = loc < capacity
            slot[k, toks[keep]] = loc[keep]
            tos[e, loc[keep]] = toks[keep]
            fill += toks.numel()
        cnt[e] = fill
    return dict(slot=slot, tos=tos, counts=cnt)


def capacity_topk(idx, logits, E, capacity):
    """top-k: expert e keeps the `capacity` largest of its column (logit if chosen else 0) over ALL S tokens, ties at the threshold in token order
    with -0.0 == +0.0 (torch.topk's comparison); a choice survives if its entry is kept; slots in token order"""
    idx = idx.cpu().long()
    K, S = idx.shape
    logits = logits.cpu().to(F64)
    slot, tos, cnt = _fill(E, capacity, S, K)
    for e in range(E):
        chosen = (idx == e).any(0)
        cnt[e] = int(chosen.sum())
        col = torch.where(chosen, logits[:, e], torch.zeros((), dtype=F64)) + 0.0
        order = torch.sort(col, descending=True, stable=True)[1]
        in_cap = torch.zeros(S, dtype=torch.bool)
        in_cap[order[:capacity]] = True
        kept = chosen & in_cap
        toks = torch.nonzero(kept).flatten()
        tos[e, :toks.numel()] = toks
        loc = torch.cumsum(kept.long(), 0) - 1
        for k in range(K):
            sel = (idx[k] == e) & kept
            slot[k, sel] = loc[sel]
    return dict(slot=slot, tos=tos, counts=cnt)


def judge_capacity(slot, tos, counts, ref, capacity):
    slot, tos = slot.cpu().long(), tos.cpu().long()
    v = [judge_equal(slot, ref["slot"], "slot"), judge_equal(tos, ref["tos"], "token_of_slot"), judge_equal(counts.cpu().long(), ref["counts"], "exp_counts")]
    if int(slot.max()) >= capacity:
        v.append((INF, f"slot {int(slot.max())} >= capacity {capacity}"))
    S = slot.shape[-1]
    kept_tokens = (slot.view(-1, S) >= 0).sum(0)                      # kept choices per token
    seen = torch.bincount(tos[tos >= 0].flatten(), minlength=S) if bool((tos >= 0).any()) else torch.zeros(S, dtype=torch.long)
    if int(tos.max()) >= S or not torch.equal(seen, kept_tokens):
        v.append((INF, "a kept choice does not appear in exactly one slot"))
    return worst(*v)


def weights_ref(gates, idx, slot):
    """g_k / max(sum of the kept g, float32 eps), float64, from a device's gates; 0 for a dropped choice"""
    idx, slot = idx.cpu().long(), slot.cpu().long()
    g = gates.cpu().to(F64).gather(1, idx.t()).t() * (slot >= 0)
    return g / g.sum(0, keepdim=True).clamp_min(EPS32)


def judge_weights(got, want, slot):
    """within 2 fp32 ulps of the float64 value (one fp32 sum of at most 16 terms and one division); exactly 0 where dropped"""
    got = got.cpu().to(F64)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 23)
    v = judge_bound(got, want, 2 * ulp, "weights")
    dropped = slot.cpu() < 0
    if bool((got[dropped] != 0).any()) or bool(torch.isnan(got).any()):
        return INF, "weights: a dropped choice has a non-zero (or NaN) weight"
    return v


def l_aux_ref(gates, idx, E, K=None):
    """E * sum_e mean_s(g) * mean_s(first choice == e); top-k (K given): every choice counts, scale E / K"""
    g = gates.cpu().to(F64)
    idx = idx.cpu().long().view(-1, g.shape[0])
    ch = idx if K is not None else idx[:1]
    ce = torch.stack([(ch == e).any(0).double().mean() for e in range(E)])
    return float((g.mean(0) * ce).sum() * (E / K if K is not None else E))


def judge_l_aux(got, want):
    f = abs(float(got) - want) / (1e-5 * abs(want)) if want != 0 and math.isfinite(float(got)) else (0.0 if float(got) == want else INF)
    return f, ("" if f <= 1 else f"l_aux {float(got)!r} vs {want!r}: {f:.3g} x 1e-5")


# ----------------------------------------------------------------------------------------------------------------------------------
# dispatch and the two combines: every step in float64, rounded to the working type
# ----------------------------------------------------------------------------------------------------------------------------------
def dispatch(x, add, mod, tos, tokens_per_sample, dt):
    """out[e][slot] = rnd(rnd(x[tok] + add[e][slot]) * mod[e][tok // tokens_per_sample]); zeros for empty slots. add [E][C][D], mod [E][B][D] or None."""
    tos = tos.cpu().long()
    E, Cc = tos.shape
    filled = tos >= 0
    a = x.to(F64)[tos.clamp_min(0)]
    if add is not None:
        a = rnd(a + add.to(F64), dt)
    if mod is not None:
        a = rnd(a * mod.to(F64)[torch.arange(E)[:, None], tos.clamp_min(0) // tokens_per_sample], dt)
    return torch.where(filled[..., None], a, torch.zeros((), dtype=F64))


def rowmap(S, rpb, bstride):
    s = torch.arange(S)
    return s if rpb <= 0 else (s // rpb) * bstride + s % rpb


def _tail(eh, ec, xs, cs, srow, prev, dt):
    if xs is not None:
        a, b = rnd(xs.to(F64)[srow] + eh, dt), rnd(cs.to(F64)[srow] + ec, dt)
        o = rnd(a + b, dt)
        mag = a.abs() + b.abs() + o.abs()
    else:
        o = rnd(eh + ec, dt)
        mag = o.abs()
    if prev is not None:
        o = rnd(prev.to(F64) + o, dt)
        mag = mag + o.abs()
    return o, mag


def combine(yh, yc, gates, idx, slot, dt, xs=None, cs=None, srow=None, prev=None):
    """top-1: rnd(rnd(xs + rnd(p yh)) + rnd(cs + rnd(p yc))), p = rnd(gate); without xs rnd(rnd(p yh) + rnd(p yc)); prev (accumulate): rnd(prev + rnd(.))"""
    idx, slot = idx.cpu().long().view(-1), slot.cpu().long().view(-1)
    S = idx.numel()
    p = rnd(gates.cpu().to(F64)[torch.arange(S), idx], dt)[:, None]
    kept = (slot >= 0)[:, None]
    zero = torch.zeros((), dtype=F64)
    eh = torch.where(kept, rnd(p * yh.to(F64)[idx, slot.clamp_min(0)], dt), zero)
    ec = torch.where(kept, rnd(p * yc.to(F64)[idx, slot.clamp_min(0)], dt), zero)
    return _tail(eh, ec, xs, cs, srow if srow is not None else torch.arange(S), prev, dt)[0]


def combine_topk(yh, yc, weights, idx, slot, dt, xs=None, cs=None, srow=None, prev=None):
    """h_k = f32(p_k y_k + h_{k-1}) over the kept choices in choice order, p = rnd(weight); one rnd; top-1's tail. Returns (out, bound): bound is 0
    where the chain is exact (bf16: the products are exact in fp32, so each step is one fp32 addition, which float64-then-fp32 reproduces) and for
    the fp32 twin 2^-22 sum_k |p_k y_k| per chain (K <= 16 fma roundings of partial sums no larger than that) plus one fp32 ulp (2^-23 |v|) of each
    value v the tail rounds after it, since a chain off by less than an ulp may round each of them the other way."""
    idx, slot = idx.cpu().long(), slot.cpu().long()
    K, S = idx.shape
    p = rnd(weights.cpu().to(F64), dt)
    D = yh.shape[-1]
    h, c = torch.zeros(S, D, dtype=F64), torch.zeros(S, D, dtype=F64)
    mag = torch.zeros(S, D, dtype=F64)
    for k in range(K):
        kept = (slot[k] >= 0)[:, None]
        ph = p[k][:, None] * yh.to(F64)[idx[k], slot[k].clamp_min(0)]
        pc = p[k][:, None] * yc.to(F64)[idx[k], slot[k].clamp_min(0)]
        h = torch.where(kept, (ph + h).to(F32).to(F64), h)
        c = torch.where(kept, (pc + c).to(F32).to(F64), c)
        mag = mag + torch.where(kept, ph.abs() + pc.abs(), torch.zeros((), dtype=F64))
    out, tail = _tail(rnd(h, dt), rnd(c, dt), xs, cs, srow if srow is not None else torch.arange(S), prev, dt)
    bound = torch.zeros_like(out) if dt == BF else 4 * U * mag + 2 * U * tail
    return out, bound


# ----------------------------------------------------------------------------------------------------------------------------------
# case tables: data, seeded and small; the CPU and GPU tests read the same cases
# ----------------------------------------------------------------------------------------------------------------------------------
def _design(n, seed, **axes):
    """n cases in which every value of every axis appears about equally often, paired at random (seeded)"""
    rng = random.Random(seed)
    cols = {}
    for name, vals in axes.items():
        col = [vals[i % len(vals)] for i in range(n)]
        rng.shuffle(col)
        cols[name] = col
    return [{k: cols[k][i] for k in cols} for i in range(n)]


GATE_S = [1, 3, 4, 5, 255, 1025]                    # four tokens per block
GATE_D = [8, 264, 512, 520, 1544, 3072]             # one trip, a ragged trip, exactly one, ragged second, ragged fourth, six whole trips of the 512-column loop
GATE_KINDS = ["even", "hot", "last", "spread", "dup", "zero"]
NOISES = ["none", "gumbel", "big"]


def gate_cases(family):
    """family: top1 | top2 | topk"""
    Es = [2, 6, 16] if family == "top2" else [1, 2, 6, 16]
    n = 24 if family == "topk" else 18
    cases = _design(n, {"top1": 11, "top2": 12, "topk": 13}[family], S=GATE_S, D=GATE_D, E=Es, ldx=[0, 64], kind=GATE_KINDS, noise=NOISES, kk=[0, 1, 2])
    # the product's widths with views into wider rows, and the longest token axis at the widest row
    cases += [dict(S=5, D=3072, E=16, ldx=64, kind="even", noise="gumbel", kk=1), dict(S=255, D=1544, E=6, ldx=64, kind="dup", noise="none", kk=2),
              dict(S=1025, D=520, E=16, ldx=64, kind="zero", noise="big", kk=2), dict(S=1025, D=3072, E=6, ldx=0, kind="spread", noise="none", kk=1)]
    out = []
    for i, c in enumerate(cases):
        E = c["E"]
        c["K"] = {"top1": 1, "top2": 2}.get(family) or [1, min(3, E), E][c.pop("kk")]
        c.pop("kk", None)
        if family != "top2":
            c["noise"] = "none"
        c["family"], c["seed"] = family, 1000 * len(family) + 7 * i + {"top1": 1, "top2": 2, "topk": 3}[family]
        c["id"] = f"{family}-{i}-S{c['S']}-D{c['D']}+{c['ldx']}-E{E}-K{c['K']}-{c['kind']}" + (f"-{c['noise']}" if family == "top2" else "")
        out.append(c)
    return out


def gate_data(c, dt):
    """-> x, c, wg in dt on the CPU, noise fp32 or None"""
    g = torch.Generator().manual_seed(c["seed"])
    S, D, E, kind = c["S"], c["D"], c["E"], c["kind"]
    x, cc = torch.randn(S, D, generator=g), torch.randn(S, D, generator=g)
    sigma = 1.0 / math.sqrt(2 * D)                                   # logits ~ N(0, 1)
    wg = torch.randn(E, D, generator=g) * sigma
    if kind == "hot":
        wg[E // 2] *= 3
    elif kind == "last":                                             # every token prefers the last expert
        x, cc = x.abs(), cc.abs()
        wg[E - 1] = 8 * sigma + 0.1 * wg[E - 1]
    elif kind == "spread":                                           # logits spread over +-80: some gates underflow to exactly 0
        wg *= 40
    elif kind == "dup" and E >= 2:                                   # two identical rows: exact ties, the lower index wins
        wg[E - 1] = wg[0]
        if E >= 6:
            wg[3] = wg[2]
    elif kind == "zero":
        for s in {0, 3, S - 1}:
            if 0 <= s < S:
                x[s], cc[s] = 0.0, 0.0
    noise = None
    if c["noise"] != "none":
        u = torch.rand(S, E, generator=g).clamp(1e-6, 1 - 1e-6)
        noise = (-torch.log(-torch.log(u)) * (20.0 if c["noise"] == "big" else 1.0)).to(F32)
    cast = (lambda t: t.to(BF)) if dt == BF else (lambda t: t.to(F32))
    return cast(x), cast(cc), cast(wg), noise


CAP_KINDS = {"rts": ["rand", "one", "unchosen", "quant"], "top2": ["rand", "one", "unchosen"],
             "topk": ["rand", "one", "unchosen", "neg", "equal", "blocks", "negzero"]}
CAPS = ["one", "oracle", "S", "S+3"]


def capacity_of(c):
    S, E, K = c["S"], c["E"], c["K"]
    return {"one": 1, "oracle": R.moe_capacity(S, E, capacity_factor=float(K)), "S": S, "S+3": S + 3}[c["cap"]]


def capacity_cases(rule):
    """hand-built idx / gates / logits / draws that the gate cannot produce"""
    out = []
    i = 0
    for kind in CAP_KINDS[rule]:
        for s_key in ["1", "2", "E-1", "1023", "1024", "1025", "2049", "4099"]:
            E = [6, 16, 3, 6][i % 4] if rule != "rts" else [6, 16, 2, 1][i % 4]
            K = {"rts": 1, "top2": 2}.get(rule) or [1, 3, E][(i // 2) % 3]
            K = min(K, E)
            if kind == "unchosen":
                E = max(E, 3)
                K = min(K, E - 1)
            S = E - 1 if s_key == "E-1" else int(s_key)
            S = max(S, 1)
            c = dict(rule=rule, kind=kind, S=S, E=E, K=K, cap=CAPS[(i + i // 4) % 4], seed=5000 + 13 * i + len(rule))
            c["id"] = f"{rule}-{kind}-S{S}-E{E}-K{K}-cap{c['cap']}"
            out.append(c)
            i += 1
    for kind in CAP_KINDS[rule]:                                     # anchors: three passes of 1024 tokens, six experts, the oracle's capacity (choices are dropped)
        K = {"rts": 1, "top2": 2}.get(rule, 3)
        c = dict(rule=rule, kind=kind, S=2049, E=6, K=K, cap="oracle", seed=6000 + len(out), anchor=True)
        c["id"] = f"{rule}-{kind}-S2049-E6-K{K}-caporacle-anchor"
        out.append(c)
    return out


def capacity_data(c):
    """-> gates fp32 [S][E], idx long [K][S] (distinct per token), logits fp32 [S][E], uniform fp32 [S][E]"""
    g = torch.Generator().manual_seed(c["seed"])
    S, E, K, kind = c["S"], c["E"], c["K"], c["kind"]
    gates = torch.softmax(torch.randn(S, E, generator=g) * 2, 1).to(F32)
    if S > 1:
        gates[1] = 0.0                                               # every kept gate exactly 0: the eps clamp decides (0 / eps = 0, not NaN)
    scores = torch.rand(S, E, generator=g)
    if kind == "one":
        scores[:, min(2, E - 1)] += 10
    if kind == "unchosen":
        scores[:, E - 1] -= 10
    idx = torch.sort(scores, 1, descending=True)[1][:, :K].t().contiguous()
    logits = ((scores - 0.5) * 4).to(F32)
    if kind == "neg":
        logits = -logits.abs() - 0.125
    elif kind == "equal":
        logits = torch.full((S, E), 0.5)
    elif kind == "blocks":                                           # equal in blocks of 700 tokens, zeros of both signs among them
        vals = torch.tensor([0.5, -0.25, 0.0, 0.5, -0.0, 2.0, 0.5])
        logits = vals[(torch.arange(S) // 700) % 7][:, None].expand(S, E).contiguous()
    elif kind == "negzero":
        logits = torch.full((S, E), -0.0)
    uniform = torch.rand(S, E, generator=g).to(F32)
    if kind == "quant":                                              # four values: the tie run at the threshold spans the 1024-token pass boundary
        uniform = torch.floor(uniform * 4) / 4
    return gates, idx, logits, uniform


def dispatch_cases():
    out = []
    tps = {1: 7, 2: 5, 3: 13}
    i = 0
    for D in (8, 520, 3072):
        for B in (1, 2, 3):
            for add, mod in ((0, 0), (1, 0), (0, 1), (1, 1)):
                if (i + B) % 2 and (add, mod) in ((1, 0), (0, 1)) and D != 520:
                    i += 1
                    continue
                out.append(dict(D=D, B=B, N=tps[B], E=[3, 4, 6][i % 3], add=add, mod=mod, seed=7000 + i, id=f"D{D}-B{B}-add{add}-mod{mod}"))
                i += 1
    return out


def dispatch_data(c, dt):
    """-> x [S][D], add [E][C][D] | None, mod [E][B][D] | None, tos [E][C] from a real routing (RTS at the oracle's capacity, empty slots present), C"""
    g = torch.Generator().manual_seed(c["seed"])
    S, E, D = c["B"] * c["N"], c["E"], c["D"]
    Cc = R.moe_capacity(S, E)
    p = torch.tensor([4.0] + [1.0] * (E - 2) + [0.2]) if E > 2 else torch.ones(E)     # uneven: an overfull expert and underfull ones
    idx = torch.multinomial(p, S, replacement=True, generator=g)
    tos = capacity_rts(idx, torch.rand(S, E, generator=g), E, Cc)["tos"]
    cast = lambda t: t.to(dt)
    x = cast(torch.randn(S, D, generator=g))
    add = cast(torch.randn(E, Cc, D, generator=g)) if c["add"] else None
    mod = cast(1 + 0.5 * torch.randn(E, c["B"], D, generator=g)) if c["mod"] else None
    return x, add, mod, tos, Cc


OPTIONS = ["plain", "resid", "mapped", "accum"]


def combine_cases():
    out = []
    i = 0
    for K in (0, 1, 2, 3, 16):                                       # 0: the top-1 combine
        for opt in OPTIONS:
            D = (8, 520, 3072)[(i + i // 4) % 3]
            out.append(dict(K=K, opt=opt, D=D, N=13 if D < 3072 else 5, E=16 if K == 16 else 5, kpad=5 if (i % 2 and K > 1) else 0, seed=9000 + i,
                            id=f"{'top1' if K == 0 else 'K%d' % K}-{opt}-D{D}-kpad{5 if (i % 2 and K > 1) else 0}"))
            i += 1
    out.append(dict(K=0, opt="resid", D=3072, N=5, E=5, kpad=0, seed=9100, id="top1-resid-D3072-kpad0"))
    out.append(dict(K=3, opt="mapped", D=3072, N=5, E=5, kpad=5, seed=9101, id="K3-mapped-D3072-kpad5"))
    return out


def combine_data(c, dt):
    """S = 3 N tokens. -> dict: yh, yc [E][C][D]; idx, slot [K][S] (top-1: [S]); weights fp32 [K][S] or gates fp32 [S][E]; sbuf [3][2N][D] whose halves
    are xs / cs when mapped, else xs, cs [S][D]; prev [S][D]. Token 1 has every choice dropped, token 2 only its last choice kept."""
    g = torch.Generator().manual_seed(c["seed"])
    K, E, D, N = max(c["K"], 1), c["E"], c["D"], c["N"]
    S = 3 * N
    idx = torch.sort(torch.rand(S, E, generator=g), 1)[1][:, :K].t().contiguous()
    slot = torch.full((K, S), -1, dtype=torch.long)
    fill = [0] * E
    for s in range(S):
        for k in range(K):
            e = int(idx[k, s])
            slot[k, s] = fill[e]
            fill[e] += 1
    Cc = max(fill) + 2
    slot[torch.rand(K, S, generator=g) < 0.25] = -1
    slot[:, 1] = -1
    slot[:-1, 2] = -1
    if slot[-1, 2] < 0:
        slot[-1, 2] = Cc - 1                                         # a free slot (the counters stop two short of Cc)
    cast = lambda t: t.to(dt)
    d = dict(S=S, C=Cc, idx=idx, slot=slot, yh=cast(torch.randn(E, Cc, D, generator=g)), yc=cast(torch.randn(E, Cc, D, generator=g)),
             prev=cast(torch.randn(S, D, generator=g)), sbuf=cast(torch.randn(3, 2 * N, D, generator=g)))
    w = torch.rand(K, S, generator=g).to(F32) * (slot >= 0)
    if K >= 3:                                                       # cancellation: on odd tokens the first two products are +-2^20 times the rest and
        for s in range(3, S, 2):                                     # sum to zero, so the chain's order decides every bit of what is left
            if bool((slot[:3, s] >= 0).all()):
                (e0, s0), (e1, s1) = [(int(idx[k, s]), int(slot[k, s])) for k in (0, 1)]
                w[1, s] = w[0, s]
                for y in (d["yh"], d["yc"]):
                    y[e0, s0] *= 2.0 ** 20
                    y[e1, s1] = -y[e0, s0]
    d["weights"] = w
    d["gates"] = torch.softmax(torch.randn(S, E, generator=g), 1).to(F32)
    if c["K"] == 0:
        d["idx"], d["slot"] = idx[0], slot[0]
    return d


def combine_ref(c, d, dt):
    """-> (want, bound) for a combine case: the option set picks the operands"""
    N, S, opt = c["N"], d["S"], c["opt"]
    kw = {}
    if opt == "resid":
        kw = dict(xs=d["sbuf"].view(-1, c["D"])[:S], cs=d["sbuf"].view(-1, c["D"])[S:2 * S])
    elif opt == "mapped":
        flat = d["sbuf"].view(-1, c["D"])
        kw = dict(xs=flat, cs=flat[N:], srow=rowmap(S, N, 2 * N))
    elif opt == "accum":
        kw = dict(prev=d["prev"])
    if c["K"] == 0:
        out = combine(d["yh"], d["yc"], d["gates"], d["idx"], d["slot"], dt, **kw)
        return out, torch.zeros_like(out)
    return combine_topk(d["yh"], d["yc"], d["weights"], d["idx"], d["slot"], dt, **kw)
