"""What the pointwise and row-glue entry points refuse before any launch, without a GPU: every entry point of csrc/elementwise.hip, objective.hip,
sana.hip, sana_bwd.hip, vae.hip, backward.hip, text.hip and depth.hip that is produced by UG_TWINS or launches pointwise_kernel, and its `_f32` twin.
Fake device addresses: each call fails an argument check, so none is dereferenced. A row is (entry, arguments, return code, who): `who` is the
first word of ug_last_error(), the name the message starts with. OWN = each twin reports its own name, FAM = both report the bf16 entry's name;
which of the two an entry does is part of its contract. The expectations were written from the UG_REQUIREs of the commit before the entry points
moved onto UG_TWINS (in their order), not from a run of the library, and the file passes on that commit's library through UG_LIB_PATH."""
import pytest

P = 1 << 20                # a fake device address, 4096-byte aligned; operand i of a call sits at (i + 1) * P where operands must differ
OK, SHAPE, ALIGN, UNSUP = 0, -1, -2, -3
OWN, FAM = "own", "family"
BIG = 1 << 62

# a valid call of each entry (its arguments but the stream), by name; a row replaces some by position
VALID = {
    "ug_cfg_combine": [P, 2 * P, 3.5, 3 * P, 64],                                         # uncond, text, gs, out, n
    "ug_euler_step": [P, 2 * P, -0.25, 64],                                               # x, v, dt, n
    "ug_add_rowbcast_f32": [P, 64, 2 * P, 64, 6, 3, 64],                                  # x, ldx, table, ldt, rows, rows_per_batch, D
    "ug_gather_rows": [P, 128, 2 * P, 3 * P, 128, 5, 128],                                # src, ld_src, idx, out, ld_out, n, W
    "ug_gather_rows_scaled": [P, 128, 2 * P, 3 * P, 128, 5, 128, 2.0],                    # ..., scale
    "ug_adaln_modulate": [P, 64, 0, 0, 2 * P, 3 * P, 64, 4, 4 * P, 64, 8, 64, 1e-6],      # x, ldx, rpb, bstride, shift, scale, mod_ld, rps, out, ldo, rows, D, eps
    # buf, ld, batches, rows_per_batch, batch_stride_rows, pos_offset, q_off, k_off, heads, dh, wq_a, wk_a, wq_b, wk_b, split, cos, sin, eps
    "ug_qk_rmsnorm_rope": [P, 512, 1, 4, 4, 0, 0, 256, 2, 128, 2 * P, 3 * P, None, None, 4, 4 * P, 5 * P, 1e-6],
    "ug_timestep_embed": [P, 2 * P, 256, 2, 256],                                         # t, out, ldo, B, dim
    "ug_pack_latents": [P, 2 * P, 1, 16, 8, 8],                                           # latents, packed, B, C, H, W
    "ug_unpack_latents": [P, 2 * P, 1, 16, 8, 8],
    # x, noise, u, sigma_table, T, scheme, pack, B, C, H, W, noisy, target, sigma, timestep, weight
    "ug_flow_noise": [P, 2 * P, 3 * P, 4 * P, 1000, 0, 0, 2, 4, 8, 8, 5 * P, 6 * P, 7 * P, 8 * P, 9 * P],
    "ug_flow_loss": [P, 2 * P, 3 * P, 2, 256, 4 * P, 5 * P, 6 * P, BIG],                  # pred, target, weight, B, n, loss_per_sample, loss, ws, ws_bytes
    "ug_flow_loss_bwd": [P, 2 * P, 3 * P, 4 * P, 2, 256, 5 * P],                          # pred, target, weight, gout, B, n, grad
    # q, k, v, o as (base, row stride, batch stride), batches, heads, N, dh, workspace
    "ug_linear_attn": [P, 384, 384 * 64, 2 * P, 384, 384 * 64, 3 * P, 384, 384 * 64, 4 * P, 128, 128 * 64, 2, 4, 64, 32, 5 * P],
    # q, k, v, dout views, state, dq, dk, dv views, batches, heads, N, dh, workspace, workspace_bytes
    "ug_linear_attn_bwd": [P, 384, 384 * 64, 2 * P, 384, 384 * 64, 3 * P, 384, 384 * 64, 4 * P, 128, 128 * 64, 5 * P, 6 * P, 384, 384 * 64, 7 * P, 384, 384 * 64,
                           8 * P, 384, 384 * 64, 2, 4, 64, 32, 9 * P, BIG],
    "ug_glu_dwconv3x3": [P, 80, 2 * P, 3 * P, 4 * P, 40, 2, 5, 7, 40],                    # x, ldx, w9, bias, out, ldo, B, H, W, C
    "ug_groupnorm_nhwc": [P, 2 * P, 3 * P, 4 * P, 5 * P, BIG, 1, 64, 64, 8, 1e-6, 0],     # x, gamma, beta, out, ws, ws_bytes, B, HW, C, G, eps, silu
    "ug_softmax_rows": [P, 64, 2 * P, 64, 4, 64, 1.0],                                    # S, ld_s, P, ld_p, rows, cols, scale
    "ug_nchw_to_nhwc": [P, 2 * P, 1, 3, 64, 8, 1.0, 0.0],                                 # in, out, B, C, HW, Cp, div, add
    "ug_nhwc_to_nchw": [P, 2 * P, 1, 3, 64, 8],
    "ug_vae_sample": [P, 32, 2 * P, 3 * P, 1, 16, 64, 0.0, 1.0],                          # mom, Cp, noise, z, B, L, HW, shift, scale
    "ug_gelu_tanh": [P, 2 * P, 64],                                                       # x, y, n
    "ug_gelu_tanh_bwd": [P, 2 * P, 3 * P, 64],                                            # x, dy, dx, n
    "ug_quick_gelu": [P, 2 * P, 64],
    "ug_gelu_erf": [P, 2 * P, 64],
    "ug_relu": [P, 2 * P, 64],
}

# (entry, {position: value}, code, who)
ROWS = [
    # elementwise.hip --- one UG_REQUIRE each for the two flat ops: everything is UG_ERR_BAD_ALIGN
    ("ug_cfg_combine", {4: 12}, ALIGN, FAM), ("ug_cfg_combine", {4: -8}, ALIGN, FAM), ("ug_cfg_combine", {0: None}, ALIGN, FAM),
    ("ug_cfg_combine", {1: 2 * P + 8}, ALIGN, FAM), ("ug_cfg_combine", {3: 3 * P + 2}, ALIGN, FAM),
    ("ug_euler_step", {3: 12}, ALIGN, FAM), ("ug_euler_step", {3: -8}, ALIGN, FAM), ("ug_euler_step", {1: None}, ALIGN, FAM),
    ("ug_euler_step", {0: P + 8}, ALIGN, FAM), ("ug_euler_step", {1: 2 * P + 4}, ALIGN, FAM),
    ("ug_add_rowbcast_f32", {4: -1}, SHAPE, FAM), ("ug_add_rowbcast_f32", {5: 0}, SHAPE, FAM), ("ug_add_rowbcast_f32", {2: None}, SHAPE, FAM),
    ("ug_add_rowbcast_f32", {6: 12}, ALIGN, FAM), ("ug_add_rowbcast_f32", {1: 68}, ALIGN, FAM), ("ug_add_rowbcast_f32", {3: 66}, ALIGN, FAM),
    ("ug_add_rowbcast_f32", {0: P + 8}, ALIGN, FAM),
    ("ug_gather_rows", {0: None}, SHAPE, FAM), ("ug_gather_rows", {2: None}, SHAPE, FAM), ("ug_gather_rows", {5: -1}, SHAPE, FAM),
    ("ug_gather_rows", {6: 12}, ALIGN, FAM), ("ug_gather_rows", {1: 132}, ALIGN, FAM), ("ug_gather_rows", {4: 132}, ALIGN, FAM),
    ("ug_gather_rows", {3: 3 * P + 8}, ALIGN, FAM),
    ("ug_gather_rows_scaled", {3: None}, SHAPE, OWN), ("ug_gather_rows_scaled", {6: -8}, SHAPE, OWN), ("ug_gather_rows_scaled", {1: 120}, SHAPE, OWN),
    ("ug_gather_rows_scaled", {4: 64}, SHAPE, OWN), ("ug_gather_rows_scaled", {6: 12, 1: 16, 4: 16}, ALIGN, OWN),
    ("ug_gather_rows_scaled", {1: 130}, ALIGN, OWN), ("ug_gather_rows_scaled", {2: 2 * P + 2}, ALIGN, OWN), ("ug_gather_rows_scaled", {0: P + 8}, ALIGN, OWN),
    ("ug_adaln_modulate", {7: 0}, SHAPE, FAM), ("ug_adaln_modulate", {4: None}, SHAPE, FAM), ("ug_adaln_modulate", {10: -1}, SHAPE, FAM),
    ("ug_adaln_modulate", {11: 12}, UNSUP, FAM), ("ug_adaln_modulate", {11: 4104}, UNSUP, FAM), ("ug_adaln_modulate", {11: 0}, UNSUP, FAM),
    ("ug_adaln_modulate", {1: 68}, ALIGN, FAM), ("ug_adaln_modulate", {6: 12}, ALIGN, FAM), ("ug_adaln_modulate", {5: 3 * P + 8}, ALIGN, FAM),
    ("ug_adaln_modulate", {8: 4 * P + 2}, ALIGN, FAM),
    ("ug_qk_rmsnorm_rope", {8: 0}, SHAPE, FAM), ("ug_qk_rmsnorm_rope", {0: None}, SHAPE, FAM), ("ug_qk_rmsnorm_rope", {7: -8}, SHAPE, FAM),
    ("ug_qk_rmsnorm_rope", {4: 3}, SHAPE, FAM), ("ug_qk_rmsnorm_rope", {5: -1}, SHAPE, FAM), ("ug_qk_rmsnorm_rope", {9: 96}, UNSUP, FAM),
    ("ug_qk_rmsnorm_rope", {1: 516}, ALIGN, FAM), ("ug_qk_rmsnorm_rope", {7: 260}, ALIGN, FAM), ("ug_qk_rmsnorm_rope", {6: 4}, ALIGN, FAM),
    ("ug_qk_rmsnorm_rope", {0: P + 8}, ALIGN, FAM), ("ug_qk_rmsnorm_rope", {16: None}, SHAPE, FAM), ("ug_qk_rmsnorm_rope", {15: 4 * P + 8}, ALIGN, FAM),
    ("ug_qk_rmsnorm_rope", {11: None}, SHAPE, FAM), ("ug_qk_rmsnorm_rope", {2: 1 << 20, 3: 1 << 10, 4: 1 << 10}, UNSUP, FAM),
    ("ug_timestep_embed", {4: 3}, SHAPE, FAM), ("ug_timestep_embed", {2: 128}, SHAPE, FAM), ("ug_timestep_embed", {0: None}, SHAPE, FAM),
    ("ug_timestep_embed", {3: -1}, SHAPE, FAM),
    # all four pack / unpack entries say ug_pack_latents
    ("ug_pack_latents", {4: 7}, SHAPE, "ug_pack_latents"), ("ug_pack_latents", {1: None}, SHAPE, "ug_pack_latents"),
    ("ug_pack_latents", {3: 1 << 20}, UNSUP, "ug_pack_latents"),
    ("ug_unpack_latents", {5: 7}, SHAPE, "ug_pack_latents"), ("ug_unpack_latents", {0: None}, SHAPE, "ug_pack_latents"),
    ("ug_unpack_latents", {2: 1 << 20}, UNSUP, "ug_pack_latents"),
    # objective.hip --- every twin reports its own name
    ("ug_flow_noise", {0: None}, SHAPE, OWN), ("ug_flow_noise", {15: None}, SHAPE, OWN), ("ug_flow_noise", {8: 0}, SHAPE, OWN),
    ("ug_flow_noise", {7: -1}, SHAPE, OWN), ("ug_flow_noise", {4: 0}, SHAPE, OWN), ("ug_flow_noise", {4: (1 << 24) + 1}, UNSUP, OWN),
    ("ug_flow_noise", {5: 99}, UNSUP, OWN), ("ug_flow_noise", {6: 2}, UNSUP, OWN), ("ug_flow_noise", {6: 1, 9: 7}, SHAPE, OWN),
    ("ug_flow_noise", {7: 65536}, UNSUP, OWN), ("ug_flow_noise", {8: 1 << 20}, UNSUP, OWN), ("ug_flow_noise", {0: P + 1}, ALIGN, OWN),
    ("ug_flow_noise", {11: 5 * P + 1}, ALIGN, OWN), ("ug_flow_noise", {2: 3 * P + 2}, ALIGN, OWN), ("ug_flow_noise", {14: 8 * P + 2}, ALIGN, OWN),
    ("ug_flow_loss", {0: None}, SHAPE, OWN), ("ug_flow_loss", {3: 0}, SHAPE, OWN), ("ug_flow_loss", {4: 0}, SHAPE, OWN),
    ("ug_flow_loss", {3: 65536}, UNSUP, OWN), ("ug_flow_loss", {4: 1 << 40}, UNSUP, OWN), ("ug_flow_loss", {1: 2 * P + 1}, ALIGN, OWN),
    ("ug_flow_loss", {2: 3 * P + 2}, ALIGN, OWN), ("ug_flow_loss", {6: None}, SHAPE, OWN), ("ug_flow_loss", {5: 4 * P + 2}, ALIGN, OWN),
    ("ug_flow_loss", {7: None}, SHAPE, OWN), ("ug_flow_loss", {8: 0}, SHAPE, OWN), ("ug_flow_loss", {7: 6 * P + 2}, SHAPE, OWN),
    ("ug_flow_loss_bwd", {2: None}, SHAPE, OWN), ("ug_flow_loss_bwd", {4: 0}, SHAPE, OWN), ("ug_flow_loss_bwd", {5: 1 << 40}, UNSUP, OWN),
    ("ug_flow_loss_bwd", {0: P + 1}, ALIGN, OWN), ("ug_flow_loss_bwd", {3: None}, SHAPE, OWN), ("ug_flow_loss_bwd", {6: None}, SHAPE, OWN),
    ("ug_flow_loss_bwd", {3: 4 * P + 2}, ALIGN, OWN), ("ug_flow_loss_bwd", {6: 5 * P + 1}, ALIGN, OWN),
    # sana.hip, sana_bwd.hip
    ("ug_linear_attn", {0: None}, SHAPE, OWN), ("ug_linear_attn", {16: None}, SHAPE, OWN), ("ug_linear_attn", {13: 0}, SHAPE, OWN),
    ("ug_linear_attn", {15: 64}, UNSUP, OWN), ("ug_linear_attn", {1: 386}, ALIGN, OWN), ("ug_linear_attn", {8: 2}, ALIGN, OWN),
    ("ug_linear_attn", {9: 4 * P + 8}, ALIGN, OWN), ("ug_linear_attn", {16: 5 * P + 8}, ALIGN, OWN), ("ug_linear_attn", {12: 65536}, UNSUP, OWN),
    ("ug_linear_attn", {14: 1 << 30}, UNSUP, OWN),
    ("ug_linear_attn_bwd", {9: None}, SHAPE, OWN), ("ug_linear_attn_bwd", {26: None}, SHAPE, OWN), ("ug_linear_attn_bwd", {12: None}, SHAPE, OWN),
    ("ug_linear_attn_bwd", {25: 64}, UNSUP, OWN), ("ug_linear_attn_bwd", {10: 130}, ALIGN, OWN), ("ug_linear_attn_bwd", {13: 6 * P + 8}, ALIGN, OWN),
    ("ug_linear_attn_bwd", {12: 5 * P + 8}, ALIGN, OWN), ("ug_linear_attn_bwd", {22: 65536}, UNSUP, OWN), ("ug_linear_attn_bwd", {27: 64}, SHAPE, OWN),
    ("ug_glu_dwconv3x3", {1: 72}, SHAPE, OWN), ("ug_glu_dwconv3x3", {5: 32}, SHAPE, OWN), ("ug_glu_dwconv3x3", {2: None}, SHAPE, OWN),
    ("ug_glu_dwconv3x3", {9: 12, 1: 24, 5: 16}, UNSUP, OWN), ("ug_glu_dwconv3x3", {1: 84}, ALIGN, OWN), ("ug_glu_dwconv3x3", {5: 44}, ALIGN, OWN),
    ("ug_glu_dwconv3x3", {3: 3 * P + 8}, ALIGN, OWN), ("ug_glu_dwconv3x3", {7: 1 << 20}, UNSUP, OWN), ("ug_glu_dwconv3x3", {6: 65536}, UNSUP, OWN),
    # vae.hip
    ("ug_groupnorm_nhwc", {9: 7}, SHAPE, FAM), ("ug_groupnorm_nhwc", {4: None}, SHAPE, FAM), ("ug_groupnorm_nhwc", {8: 12, 9: 3}, UNSUP, FAM),
    ("ug_groupnorm_nhwc", {8: 1024, 9: 2}, UNSUP, FAM), ("ug_groupnorm_nhwc", {0: P + 8}, ALIGN, FAM), ("ug_groupnorm_nhwc", {4: 5 * P + 4}, ALIGN, FAM),
    ("ug_groupnorm_nhwc", {5: 0}, SHAPE, FAM), ("ug_groupnorm_nhwc", {6: 65536}, UNSUP, FAM),
    ("ug_softmax_rows", {1: 32}, SHAPE, FAM), ("ug_softmax_rows", {3: 32}, SHAPE, FAM), ("ug_softmax_rows", {2: None}, SHAPE, FAM),
    ("ug_softmax_rows", {5: 0}, SHAPE, FAM), ("ug_softmax_rows", {4: 1 << 31}, SHAPE, FAM),
    ("ug_nchw_to_nhwc", {5: 2}, SHAPE, FAM), ("ug_nchw_to_nhwc", {0: None}, SHAPE, FAM), ("ug_nchw_to_nhwc", {4: 1 << 31}, SHAPE, FAM),
    ("ug_nhwc_to_nchw", {5: 2}, SHAPE, FAM), ("ug_nhwc_to_nchw", {1: None}, SHAPE, FAM), ("ug_nhwc_to_nchw", {3: 0}, SHAPE, FAM),
    ("ug_vae_sample", {1: 31}, SHAPE, FAM), ("ug_vae_sample", {2: None}, SHAPE, FAM), ("ug_vae_sample", {6: 1 << 31}, SHAPE, FAM),
    # backward.hip: ug_gelu_tanh_bwd says ug_gelu_tanh; any n and alignment is served, so only null pointers and a negative n are refused
    ("ug_gelu_tanh", {0: None}, SHAPE, "ug_gelu_tanh"), ("ug_gelu_tanh", {1: None}, SHAPE, "ug_gelu_tanh"), ("ug_gelu_tanh", {2: -1}, SHAPE, "ug_gelu_tanh"),
    ("ug_gelu_tanh_bwd", {0: None}, SHAPE, "ug_gelu_tanh"), ("ug_gelu_tanh_bwd", {2: None}, SHAPE, "ug_gelu_tanh"),
    ("ug_gelu_tanh_bwd", {3: -13}, SHAPE, "ug_gelu_tanh"),
    # text.hip
    ("ug_quick_gelu", {0: None}, SHAPE, OWN), ("ug_quick_gelu", {2: -8}, SHAPE, OWN), ("ug_quick_gelu", {2: 12}, UNSUP, OWN),
    ("ug_quick_gelu", {0: P + 8}, ALIGN, OWN), ("ug_quick_gelu", {1: 2 * P + 2}, ALIGN, OWN), ("ug_quick_gelu", {2: 8 * 256 << 31}, UNSUP, OWN),
    ("ug_gelu_erf", {1: None}, SHAPE, OWN), ("ug_gelu_erf", {2: -8}, SHAPE, OWN), ("ug_gelu_erf", {2: 13}, UNSUP, OWN),
    ("ug_gelu_erf", {0: P + 4}, ALIGN, OWN), ("ug_gelu_erf", {1: 2 * P + 8}, ALIGN, OWN), ("ug_gelu_erf", {2: 8 * 256 << 31}, UNSUP, OWN),
    # depth.hip: one UG_REQUIRE, UG_ERR_BAD_SHAPE; a base off 16 bytes is served (the guarded path), so it is no refusal
    ("ug_relu", {0: None}, SHAPE, FAM), ("ug_relu", {1: None}, SHAPE, FAM), ("ug_relu", {2: 12}, SHAPE, FAM), ("ug_relu", {2: -8}, SHAPE, FAM),
    ("ug_relu", {2: 8 * 256 << 31}, SHAPE, FAM),
]
# served without a launch: nothing to do
EMPTY = [("ug_cfg_combine", {4: 0}), ("ug_euler_step", {3: 0}), ("ug_add_rowbcast_f32", {4: 0}), ("ug_gather_rows", {5: 0}), ("ug_gather_rows_scaled", {6: 0}),
         ("ug_adaln_modulate", {10: 0}), ("ug_qk_rmsnorm_rope", {2: 0}), ("ug_timestep_embed", {3: 0}), ("ug_pack_latents", {2: 0}), ("ug_unpack_latents", {2: 0}),
         ("ug_flow_noise", {7: 0}), ("ug_linear_attn", {14: 0}), ("ug_linear_attn_bwd", {24: 0}), ("ug_glu_dwconv3x3", {6: 0}), ("ug_groupnorm_nhwc", {7: 0}),
         ("ug_softmax_rows", {4: 0}), ("ug_nchw_to_nhwc", {2: 0}), ("ug_nhwc_to_nchw", {2: 0}), ("ug_vae_sample", {4: 0}), ("ug_gelu_tanh", {2: 0}),
         ("ug_gelu_tanh_bwd", {3: 0}), ("ug_quick_gelu", {2: 0}), ("ug_gelu_erf", {2: 0}), ("ug_relu", {2: 0})]


def _call(cdll, entry, twin, patch):
    args = list(VALID[entry])
    for pos, val in patch.items():
        args[pos] = val
    return getattr(cdll, entry + ("_f32" if twin else ""))(*args, None)


def _id(row):
    return f"{row[0]}-{'-'.join(f'{k}={v}' for k, v in row[1].items())}"


@pytest.mark.parametrize("twin", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_refused_before_launch(row, twin):
    from unigen_amd import lib
    entry, patch, code, who = row
    cdll = lib.load()
    assert (OK, SHAPE, ALIGN, UNSUP) == (lib.UG_OK, lib.UG_ERR_BAD_SHAPE, lib.UG_ERR_BAD_ALIGN, lib.UG_ERR_UNSUPPORTED)
    rc = _call(cdll, entry, twin, patch)
    msg = cdll.ug_last_error().decode()
    want = {OWN: entry + ("_f32" if twin else ""), FAM: entry}.get(who, who)
    assert rc == code, (entry, twin, patch, rc, msg)
    assert msg.split(":")[0] == want, (entry, twin, patch, msg)


@pytest.mark.parametrize("twin", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("row", EMPTY, ids=_id)
def test_empty_is_ok_without_a_launch(row, twin):
    from unigen_amd import lib
    assert _call(lib.load(), row[0], twin, row[1]) == lib.UG_OK


def test_tile_blend_null_descriptor():
    from unigen_amd import lib
    cdll = lib.load()
    for fn in (cdll.ug_vae_tile_blend, cdll.ug_vae_tile_blend_f32):
        assert fn(None, None) == lib.UG_ERR_BAD_SHAPE and cdll.ug_last_error().startswith(b"ug_vae_tile_blend: null descriptor")


def test_every_rewritten_entry_has_rows():
    assert {r[0] for r in ROWS} == set(VALID) and {r[0] for r in EMPTY} | {"ug_flow_loss", "ug_flow_loss_bwd"} == set(VALID)
