"""The refusals of every C entry point that takes attention operands as (pointer, row stride, batch stride) views, without a GPU
(include/unigen_hip.h, "Strided attention views"; fake aligned pointers, as tests/test_sana_bwd_code_object_cpu.py).

No call here may reach a launch. So the call every case starts from is not a valid one but one that passes every check except the LAST of its
entry point - the grid limit - and is refused there ("... too large"): a perturbed field that the entry point accepts shows as that same late
refusal, one that it refuses shows as an earlier code, and every single violation is at the same time a statement about precedence (it wins over
the grid limit). The expected codes are the table of the header, written down in ENTRIES from the code of the commit before the shared checker
existed; the file passes against that commit's library unchanged (UG_LIB_PATH)."""
import pytest

P = 4096                    # a fake device address, 4096-byte aligned
RS, BS = 1024, 64 * 1024    # row / batch stride (elements) of every view of the starting call: multiples of 8, wider than heads x dh everywhere
BIG = 1 << 31               # batches of the starting call: the grid no entry point accepts
LIMIT = 1 << 24

_FWD = ("q", "k", "v", "o")
_BWD = ("q", "k", "v", "o", "do", "dq", "dk", "dv")
_LAB = ("q", "k", "v", "do", "dq", "dk", "dv")


def _rules(names, mult, align, bounded=()):
    """{view: (stride multiple in elements, base alignment in bytes, row stride bounded to (0, 2^24))}; mult / align: one value or {view: value}"""
    get = lambda x, n: x.get(n, x["*"]) if isinstance(x, dict) else x
    return {n: (get(mult, n), get(align, n), n in bounded) for n in names}


# entry -> what its table line says. `tail`: the arguments after the views, in order; `dh`: an accepted head width; the counts whose zero
# means "nothing to do" (UG_OK before any pointer is looked at) are batches and Lq / N; `bufs`: plain buffers, with the code a base 8 bytes off a
# 16-byte boundary gets (the attention backward counts that as "no workspace"); `start`: fields of the starting call
ENTRIES = {
    "fwd": dict(fn="ug_flash_attn_fwd", views=_rules(_FWD, {"*": 8, "o": 4}, {"*": 16, "o": 8}, _FWD),
                tail=("batches", "heads", "Lq", "Lkv", "dh", "scale"), dh=128),
    "fwd_lse": dict(fn="ug_flash_attn_fwd_lse", views=_rules(_FWD, {"*": 8, "o": 4}, {"*": 16, "o": 8}, _FWD),
                    tail=("batches", "heads", "Lq", "Lkv", "dh", "scale", "lse2", "lse_ld"), dh=64),
    "fwd_f32": dict(fn="ug_flash_attn_fwd_f32", views=_rules(_FWD, 4, 16), tail=("batches", "heads", "Lq", "Lkv", "dh", "scale"), dh=128),
    "fwd_wide": dict(fn="ug_flash_attn_fwd_wide", views=_rules(_FWD, {"*": 8, "o": 4}, {"*": 16, "o": 8}, ("k", "v")),
                     tail=("batches", "heads", "Lq", "Lkv", "dh", "scale"), dh=512),
    "fwd_wide_f32": dict(fn="ug_flash_attn_fwd_wide_f32", views=_rules(_FWD, 4, 16), tail=("batches", "heads", "Lq", "Lkv", "dh", "scale"), dh=512),
    "bwd": dict(fn="ug_flash_attn_bwd", views=_rules(_BWD, 8, {"*": 16, "dq": 8, "dk": 8, "dv": 8}, _BWD),
                tail=("batches", "heads", "Lq", "Lkv", "dh", "scale", "lse_in", "ws", "ws_bytes"), dh=128, bufs={"ws": "UG_ERR_BAD_SHAPE"}),
    "linear": dict(fn="ug_linear_attn", views=_rules(_FWD, 8, 16), tail=("batches", "heads", "N", "dh", "ws"), dh=32, bufs={"ws": "UG_ERR_BAD_ALIGN"}),
    "linear_f32": dict(fn="ug_linear_attn_f32", views=_rules(_FWD, 4, 16), tail=("batches", "heads", "N", "dh", "ws"), dh=32, bufs={"ws": "UG_ERR_BAD_ALIGN"}),
    "linear_bwd": dict(fn="ug_linear_attn_bwd", views=_rules(_LAB, 8, 16), tail=("batches", "heads", "N", "dh", "ws", "ws_bytes"), dh=32,
                       bufs={"state": "UG_ERR_BAD_ALIGN", "ws": "UG_ERR_BAD_ALIGN"}),
    "linear_bwd_f32": dict(fn="ug_linear_attn_bwd_f32", views=_rules(_LAB, 4, 16), tail=("batches", "heads", "N", "dh", "ws", "ws_bytes"), dh=32,
                           bufs={"state": "UG_ERR_BAD_ALIGN", "ws": "UG_ERR_BAD_ALIGN"}),
}
_BIAS_TAIL = ("batches", "heads", "Lq", "Lkv", "dh", "scale", "rel_table", "rel_len", "causal")
for _mode, _kw in (("table", dict(rel_table=P, causal=0)), ("causal", dict(rel_table=None, causal=1)), ("both", dict(rel_table=P, causal=1))):
    ENTRIES[f"fwd_bias[{_mode}]"] = dict(fn="ug_flash_attn_fwd_bias", views=_rules(_FWD, {"*": 8, "o": 4}, {"*": 16, "o": 8}), tail=_BIAS_TAIL, dh=64, start=_kw)
    ENTRIES[f"fwd_bias_f32[{_mode}]"] = dict(fn="ug_flash_attn_fwd_bias_f32", views=_rules(_FWD, 4, 16), tail=_BIAS_TAIL, dh=64, start=_kw)
# neither table nor mask: the two entries ARE ug_flash_attn_fwd / _fwd_f32, row-stride bound included
ENTRIES["fwd_bias[plain]"] = dict(ENTRIES["fwd"], fn="ug_flash_attn_fwd_bias", tail=_BIAS_TAIL, start=dict(rel_table=None, causal=0))
ENTRIES["fwd_bias_f32[plain]"] = dict(ENTRIES["fwd_f32"], fn="ug_flash_attn_fwd_bias_f32", tail=_BIAS_TAIL, start=dict(rel_table=None, causal=0))


@pytest.fixture(scope="module")
def L():
    from unigen_amd import lib
    lib.load()
    return lib


def _start(e):
    a = dict(batches=BIG, heads=2, Lq=64, Lkv=64, N=64, dh=e["dh"], scale=0.125, lse2=P, lse_ld=64, lse_in=None, ws=P, ws_bytes=1 << 62, state=P,
             rel_table=P, rel_len=64, causal=0)
    a.update(e.get("start", {}))
    for n in e["views"]:
        a[n], a[n + "_rs"], a[n + "_bs"] = P, RS, BS
    return a


def _call(L, e, **kw):
    a = _start(e)
    assert set(kw) <= set(a), kw
    a.update(kw)
    args = []
    for n in e["views"]:
        if e["fn"].startswith("ug_linear_attn_bwd") and n == "dq":
            args.append(a["state"])                        # the one entry whose views are not contiguous in the argument list
        args += [a[n], a[n + "_rs"], a[n + "_bs"]]
    rc = getattr(L.load(), e["fn"])(*args, *(a[t] for t in e["tail"]), None)
    return rc, L.load().ug_last_error()


def _expect(L, e, want, kw):
    """want: a code, (code, bytes the message must hold), or "late": accepted as far as the entry point's last check, the grid limit"""
    rc, msg = _call(L, e, **kw)
    code, text = (L.UG_ERR_UNSUPPORTED, b"too large") if want == "late" else want if isinstance(want, tuple) else (want, b"")
    assert rc == code and text in msg, (e["fn"], kw, want, rc, msg)
    if want == "late":
        assert b"2^24" not in msg, (e["fn"], kw, msg)


def _work(e):
    return ("batches", "N") if "N" in e["tail"] else ("batches", "Lq")


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_single_violations(L, name):
    e = ENTRIES[name]
    _expect(L, e, "late", {})                                                                  # the starting call itself
    RANGE = (L.UG_ERR_UNSUPPORTED, b"2^24")
    for v, (mult, align, bounded) in e["views"].items():
        for off in (8, 4):                                                                     # the base
            _expect(L, e, L.UG_ERR_BAD_ALIGN if off % align else "late", {v: P + off})
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {v: P + 2})
        for s in ("_rs", "_bs"):                                                               # each stride off its multiple, and on it
            _expect(L, e, L.UG_ERR_BAD_ALIGN, {v + s: RS + mult // 2})
            _expect(L, e, "late", {v + s: RS + mult})
        if bounded:                                                                            # the row stride's range
            for rs in (0, -8, LIMIT):
                _expect(L, e, RANGE, {v + "_rs": rs})
            _expect(L, e, "late", {v + "_rs": LIMIT - 8})
        else:
            _expect(L, e, "late", {v + "_rs": LIMIT})
        _expect(L, e, "late", {v + "_bs": LIMIT})                                              # no batch stride is bounded
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {v: None})
    for b, misaligned in e.get("bufs", {}).items():
        _expect(L, e, getattr(L, misaligned), {b: P + 8})
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {b: None})
    for c in e["tail"]:
        if c in _work(e):
            _expect(L, e, L.UG_OK, {c: 0})
            _expect(L, e, L.UG_ERR_BAD_SHAPE, {c: -1})
        elif c in ("heads", "Lkv"):
            _expect(L, e, L.UG_ERR_BAD_SHAPE, {c: 0})
            _expect(L, e, L.UG_ERR_BAD_SHAPE, {c: -2})
    _expect(L, e, (L.UG_ERR_UNSUPPORTED, b"head dim"), {"dh": 96})


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_precedence(L, name):
    e = ENTRIES[name]
    views = list(e["views"])
    DH, RANGE = (L.UG_ERR_UNSUPPORTED, b"head dim"), (L.UG_ERR_UNSUPPORTED, b"2^24")
    for c in _work(e):                                                                         # nothing to do: before any pointer is looked at
        _expect(L, e, L.UG_OK, {c: 0, "q": None})
        _expect(L, e, L.UG_OK, {c: 0, views[-1]: P + 2, "heads": -1, "dh": 96})
    for v in views:                                                                            # shape, then head width, then alignment
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {v: None, "dh": 96})
        _expect(L, e, DH, {v: P + 2, "dh": 96})
        _expect(L, e, DH, {v + "_rs": RS + 1, "dh": 96})
    bounded = [v for v in views if e["views"][v][2]]
    for v in bounded:                                                                          # alignment of ANY view before the range of any
        for w in views:
            _expect(L, e, L.UG_ERR_BAD_ALIGN, {v + "_rs": LIMIT, w + "_bs": RS + 1})
            if w != v:
                _expect(L, e, L.UG_ERR_BAD_ALIGN, {v + "_rs": -8, w: P + 2})
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {v + "_rs": LIMIT + 1})
    if "Lkv" in e["tail"]:                                                                     # the sequence length: UNSUPPORTED before alignment
        _expect(L, e, (L.UG_ERR_UNSUPPORTED, b"sequence too long"), {"Lkv": 1 << 30, "q": P + 2})
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {"Lkv": 1 << 30, "q": None})
    else:                                                                                      # linear attention: "too large" after alignment
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {"N": 1 << 30, "q": P + 8})
    if name in ("fwd_lse",):                                                                   # lse2 / lse_ld first of all
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {"Lq": 0, "lse2": None})
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {"batches": 0, "lse_ld": 63})
        _expect(L, e, L.UG_OK, {"Lq": 0, "lse_ld": 0})
    if name == "fwd_wide":                                                                     # range, then the scale, then the grid
        _expect(L, e, (L.UG_ERR_UNSUPPORTED, b"softmax_scale"), {"scale": 0.0})
        _expect(L, e, RANGE, {"scale": 0.0, "k_rs": LIMIT})
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {"scale": -1.0, "o": P + 4})
    if name == "bwd":                                                                          # range, then the workspace, then the grid
        short = 2 * 2 * 2 * 64 * 4 - 16
        _expect(L, e, (L.UG_ERR_BAD_SHAPE, b"workspace"), {"ws_bytes": short})
        _expect(L, e, (L.UG_ERR_BAD_SHAPE, b"workspace"), {"ws_bytes": short, "batches": 2})
        _expect(L, e, (L.UG_ERR_BAD_SHAPE, b"workspace"), {"ws": P + 8, "batches": 2})
        for v in bounded:
            _expect(L, e, RANGE, {"ws_bytes": short, "batches": 2, v + "_rs": LIMIT})
            _expect(L, e, RANGE, {"ws": None, v + "_rs": 0})
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {"ws_bytes": short, "dv": P + 4})
    if name.startswith("linear_bwd"):                                                          # shape, state, head width, alignment, size, workspace
        _expect(L, e, (L.UG_ERR_BAD_SHAPE, b"state"), {"state": None, "dh": 96})
        _expect(L, e, L.UG_ERR_BAD_SHAPE, {"state": None, "q": None})
        _expect(L, e, DH, {"state": P + 8, "dh": 96})
        state = (32 * 32 + 32) * 4
        _expect(L, e, (L.UG_ERR_BAD_SHAPE, b"workspace"), {"batches": 2, "ws_bytes": 2 * 2 * 2 * state - 16})
        _expect(L, e, "late", {"ws_bytes": 0})
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {"batches": 2, "ws_bytes": 0, "dk": P + 8})
    if e["fn"].startswith("ug_flash_attn_fwd_bias") and "plain" not in name:                   # shape, sequence, table, head width, alignment, grid
        if e["start"]["rel_table"]:
            _expect(L, e, (L.UG_ERR_BAD_SHAPE, b"rel_len"), {"rel_len": 63, "dh": 128, "q": P + 2})
            _expect(L, e, (L.UG_ERR_UNSUPPORTED, b"rel_len"), {"rel_len": 4097, "q": P + 2})
            _expect(L, e, (L.UG_ERR_BAD_ALIGN, b"rel_table"), {"rel_table": P + 2, "dh": 128})
            _expect(L, e, (L.UG_ERR_UNSUPPORTED, b"sequence too long"), {"Lkv": 1 << 30, "rel_len": 63})
        _expect(L, e, DH, {"dh": 128})                                                         # 64 only with a bias or a mask
        _expect(L, e, DH, {"dh": 128, "o": P + 2})
    if "plain" in name:
        _expect(L, e, "late", {"dh": 64 if e["dh"] == 128 else 128})


def test_the_o_distinction(L):
    """o is written with 8-byte stores by the bf16 forwards (base 8-byte aligned, strides multiples of 4) and with 16-byte accesses by the fp32 twins
    and read with 16-byte loads by the backward"""
    for name, e in ENTRIES.items():
        if "o" not in e["views"]:
            continue
        narrow = e["fn"] in ("ug_flash_attn_fwd", "ug_flash_attn_fwd_lse", "ug_flash_attn_fwd_wide", "ug_flash_attn_fwd_bias")
        _expect(L, e, "late" if narrow else L.UG_ERR_BAD_ALIGN, {"o": P + 8})
        bf16_mult4 = narrow or e["views"]["o"][0] == 4
        _expect(L, e, "late" if bf16_mult4 else L.UG_ERR_BAD_ALIGN, {"o_rs": RS + 4})
        _expect(L, e, "late" if bf16_mult4 else L.UG_ERR_BAD_ALIGN, {"o_bs": BS + 4})
        _expect(L, e, L.UG_ERR_BAD_ALIGN, {"o": P + 4})
