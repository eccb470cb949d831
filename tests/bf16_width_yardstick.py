"""The yardstick behind the bf16 bounds of tests/test_model_shapes_gpu.py: the oracle with weights and activations rounded to
bf16 (torch.autocast on the CPU) against the fp32 oracle, on the batches and weights that test uses.  CPU only, a few seconds:

    python tests/bf16_width_yardstick.py [kind ...]

A bound that a configuration's HIP result does not meet at the project's starting values is twice the figure printed here."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import deepsvg_amd                                              # noqa: E402
from oracle import svg_transformer_oracle as O                  # noqa: E402
from tests import helpers as H                                  # noqa: E402


def measure(kind, seed=2024, wseed=777, eps_seed=2101):
    cfg = H.build_cfg(kind)
    n = 6 if kind == "wide512" else 8
    commands, args, args_dec = H.width_batch(cfg, kind, n, seed=seed)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), wseed)
    eps = torch.randn(1, 1, n, cfg.dim_z, generator=torch.Generator().manual_seed(eps_seed)) if cfg.use_vae else None
    o_out, o_ld, o_grads = O.loss_and_grads(sd, cfg, commands, args, O.DEFAULT_WEIGHTS, eps=eps, args_dec=args_dec)
    sdb = {k: (v.bfloat16().float() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16):
        b_out, b_ld, b_grads = O.loss_and_grads(sdb, cfg, commands, args, O.DEFAULT_WEIGHTS, eps=eps, args_dec=args_dec)
    e_c = (b_out["command_logits"].float() - o_out["command_logits"]).abs().max().item()
    e_a = (b_out["args_logits"].float() - o_out["args_logits"]).abs().max().item()
    same = b_out["command_logits"].argmax(-1) == o_out["command_logits"].argmax(-1)
    lrel = max(abs(b_ld[k].item() - o_ld[k].item()) / max(1.0, abs(o_ld[k].item())) for k in o_ld)
    names = [k for k in o_grads if o_grads[k] is not None and o_grads[k].norm() > 0]
    norm = lambda t: t.double().norm().item()                   # noqa: E731
    rel = sorted(abs(norm(b_grads[k]) - norm(o_grads[k])) / max(norm(o_grads[k]), 1e-8) for k in names)
    d = sorted(H.rel_l2(b_grads[k].float(), o_grads[k]) for k in names)
    return (f"{kind}: command_logits max abs {e_c:.3e} (argmax agree {same.float().mean().item():.4f}, {int(same.sum())} of "
            f"{same.numel()}), args_logits max abs {e_a:.3e}, worst loss-term rel {lrel:.3e}, grad-norm rel median "
            f"{rel[len(rel) // 2]:.3e} max {rel[-1]:.3e}, gradient direction median {d[len(d) // 2]:.3e} p90 "
            f"{d[int(0.9 * len(d))]:.3e} worst {d[-1]:.3e}")


if __name__ == "__main__":
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    for kind_ in sys.argv[1:] or H.WIDTH_KINDS:
        print(measure(kind_), flush=True)
