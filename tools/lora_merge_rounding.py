"""Why the LoRA merge rounds once: the same adapter merged into the same tiny UniGenFlux three ways, each forward held against the fp32 CPU oracle on
HOST-merged weights (tests/lora_io_ref.py `merge_ref`, rounded to bf16):
  host      a plain model loaded with the host-merged weights;
  aliased   ONE ug_gemm launch per weight, UG_EPI_RES_SCALE with the residual aliased to the output - that epilogue rounds the product to bf16 before
            it adds the residual, so the weight is rounded twice;
  shipped   HipModule.fuse_lora: the product through the fp32 epilogue, then ug_add_rowbcast_f32 - one rounding.
Model, inputs and adapter are those of tests/test_lora_io_gpu.py.
    python tools/lora_merge_rounding.py"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from oracle import unigen_ref as R
from tests import lora_io_ref as LR
import tests.test_lora_io_gpu as G
from tests.test_flux_gpu import TINY, _to_dev
from tests.util import rel_l2
from unigen_amd import lib as L, ops

BF, gpu = torch.bfloat16, torch.device("cuda:0")
model = G._flux(gpu, BF)
state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
rcfg = R.FluxConfig(condition_nums=1, **TINY)
inp = R.make_inputs(rcfg, B=2, grid=8, T=32)
t = torch.full((2,), 0.75, dtype=BF)
dinp = {k: _to_dev(v, gpu) for k, v in inp.items()}
bfl, canon = G.flux_adapter(state)
m16 = LR.merged_state(state, canon, BF)
run = lambda st, dt: R.unigen_flux_forward(st, rcfg, timestep=t, dtype=dt, **inp)[0]
truth, ref16 = run(m16, torch.float32), run(m16, BF)
fw = lambda m: m(timestep=t.to(gpu), **dinp)[0]


def differs(m):
    sd = m.state_dict()
    n = sum(int((sd[k + ".weight"].cpu() != m16[k + ".weight"]).sum()) for k in canon)
    return n / sum(m16[k + ".weight"].numel() for k in canon)


res = dict(err_oracle_bf16=rel_l2(ref16, truth))
res["tolerance"] = 1.25 * res["err_oracle_bf16"] + 1e-3
host = G._flux(gpu, BF, m16)
res["host"] = dict(err=rel_l2(fw(host), truth), weight_elements_differing_from_host_merge=differs(host))
aliased = G._flux(gpu, BF, state)
for k, e in canon.items():
    w = aliased.get_parameter(k + ".weight").data
    r = e[0].shape[0]
    Ac = torch.zeros(64, w.shape[1], device=gpu, dtype=BF); Ac[:r] = e[0].to(gpu, BF)
    Bs = torch.zeros(w.shape[0], 64, device=gpu, dtype=BF); Bs[:, :r] = (e[1].to(gpu, BF).float() * LR.scaling(e)).to(BF)
    ops.gemm(Bs, ops.transpose(Ac), None, w, M=w.shape[0], epilogue=L.EPI_RES_SCALE, residual=w, alpha=1.0)
res["aliased_res_scale"] = dict(err=rel_l2(fw(aliased), truth), weight_elements_differing_from_host_merge=differs(aliased))
model.load_lora_weights(LR.write_kohya(bfl), adapter_name="style")
model.fuse_lora()
res["shipped"] = dict(err=rel_l2(fw(model), truth), weight_elements_differing_from_host_merge=differs(model))
print("LORA_MERGE_ROUNDING", json.dumps(res))
