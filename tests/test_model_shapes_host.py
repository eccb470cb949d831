"""Configurations off the default width (tests/helpers.py WIDTH_KINDS) on the host: which of them construct, and - with
deepsvg_amd.ops replaced by the plain-torch restatements - that the model's host logic (layouts, flat parameter store,
the "does this layer fit a fused kernel" decisions) reproduces the oracle at every one of them."""
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import config as C
from oracle import svg_transformer_oracle as O
from tests import helpers as H


@pytest.mark.parametrize("kind", H.WIDTH_KINDS)
def test_width_kinds_construct(kind):
    cfg = H.build_cfg(kind)
    assert cfg.d_model == 32 * cfg.n_heads
    model = deepsvg_amd.SVGTransformer(cfg)
    assert sum(p.numel() for p in model.parameters()) > 0


def test_six_and_three_heads_construct_at_every_supported_length():
    """the attention dispatch ends in a one-head-per-workgroup instantiation (csrc/attention.hip, <64,1>), so a head count
    that is neither a multiple of 8 nor of 4 has a kernel at 33..64 tokens too, and an odd one at every length; beyond 64
    tokens the long-sequence kernels run one workgroup per (sequence, head).  tests/test_attention_heads_gpu.py and
    tests/test_model_shapes_gpu.py (odd192, odd192_1s, odd96) run them."""
    cfg = H.build_cfg("odd192")                 # two stages, 22 tokens
    assert (cfg.n_heads, cfg.max_seq_len, cfg.encode_stages) == (6, 20, 2)
    deepsvg_amd.SVGTransformer(cfg)
    cfg = H.build_cfg("odd192_1s")              # one stage, 52 tokens
    assert (cfg.n_heads, cfg.max_total_len, cfg.encode_stages) == (6, 50, 1)
    deepsvg_amd.SVGTransformer(cfg)
    cfg = H.build_cfg("odd96")                  # 3 heads
    assert cfg.n_heads == 3
    deepsvg_amd.SVGTransformer(cfg)
    cfg.max_seq_len = 100                       # 102-token paths
    deepsvg_amd.SVGTransformer(cfg)


def test_head_dim_other_than_32_is_refused():
    cfg = C.Hierarchical()
    cfg.n_heads = 4                             # d_model 256: head_dim 64
    with pytest.raises(NotImplementedError, match="head_dim == 32"):
        deepsvg_amd.SVGTransformer(cfg)
    cfg = C.Hierarchical()
    cfg.d_model, cfg.n_heads = 200, 6           # 200 // 6 == 33
    with pytest.raises(NotImplementedError, match="head_dim == 32"):
        deepsvg_amd.SVGTransformer(cfg)
    cfg = C.OneStageOneShot()
    cfg.d_model, cfg.n_heads, cfg.max_total_len = 192, 6, 300
    with pytest.raises(NotImplementedError, match="at most 256 tokens"):
        deepsvg_amd.SVGTransformer(cfg)


@pytest.mark.parametrize("kind", H.WIDTH_KINDS)
def test_width_kinds_match_the_oracle_with_emulated_ops(kind, emulated_ops):
    cfg = H.build_cfg(kind)
    n = 4
    # (seed 31 puts one pre-activation of ff1024's last FFN within fp32 rounding of zero: its ReLU gate then differs from
    # the oracle's and every gradient below it moves by 7e-4 - a property of the batch, measured against a float64 oracle)
    commands, args, args_dec = H.width_batch(cfg, kind, n, seed=33)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 77)
    eps = torch.randn(1, 1, n, cfg.dim_z, generator=torch.Generator().manual_seed(3)) if cfg.use_vae else None
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(sd)
    model.eval()
    import deepsvg_amd.model as M
    orig = torch.randn_like
    if eps is not None:
        M.torch.randn_like = lambda t: eps.reshape(t.shape).to(t.dtype)
    try:
        out = model(commands, args, commands, args_dec, params={})
        ld = deepsvg_amd.SVGLoss(cfg)(out, None, weights=O.DEFAULT_WEIGHTS)
        ld["loss"].backward()
    finally:
        M.torch.randn_like = orig
    o_out, o_ld, o_grads = O.loss_and_grads(sd, cfg, commands, args, eps=eps, args_dec=args_dec)
    for k in ("command_logits", "args_logits", "visibility_logits"):
        if k in o_out:
            assert torch.allclose(out[k].detach(), o_out[k].detach(), rtol=1e-4, atol=1e-5), k
    for k in o_ld:
        assert abs(float(ld[k].detach()) - o_ld[k].item()) <= 1e-5 * max(1.0, abs(o_ld[k].item())), k
    grads = {n_: p.grad for n_, p in model.named_parameters()}
    worst, name = max((H.rel_l2(grads[n_], o_grads[n_]), n_) for n_ in o_grads if o_grads[n_] is not None)
    assert worst < 2e-4, (worst, name)
    if cfg.self_match:
        assert torch.equal(model.last_assignment.long(), o_out["_assignment"].long())
