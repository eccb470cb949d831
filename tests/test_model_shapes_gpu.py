"""The whole model off the default width (tests/helpers.py WIDTH_KINDS: d_model 96 .. 512, 3 .. 16 heads, dim_feedforward 192 ..
1024, other group counts and path lengths, no latent ResNet) on a real MI355X against the CPU oracle.  None of these
configurations fits a fused kernel completely: the "does not fit, take the general kernels" side of every shape test in
ParamStore / functional runs here end to end, the mixed layer (fused attention, unfused FFN) included."""
import functools

import pytest
import torch

import deepsvg_amd
import deepsvg_amd.functional as Fn
from deepsvg_amd import ops
from oracle import svg_transformer_oracle as O
from tests import helpers as H
from tests.test_model_gpu import BF16_DIR_BOUNDS, DEV, _check_grad_directions, _fwd_bwd, _hip_model, _parity_log

pytestmark = pytest.mark.gpu

KINDS = list(H.WIDTH_KINDS)
WSEED = 777
FUSED_OPS = ("ffn_fwd", "attn_block_fwd", "gs_layer_fwd", "gs_stack_fwd")


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """tests that run later measure how much device memory an op allocates (tests/test_draw_grad_gpu.py and its kind): a
    free block this file leaves in torch's caching allocator would be handed to them whole, slack included"""
    yield
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _n_icons(kind):
    return 6 if kind == "wide512" else 8


@functools.lru_cache(maxsize=None)
def _case(kind):
    """-> (cfg, state dict, commands, args, args_dec, eps, oracle outputs, oracle losses, oracle gradients): computed once per
    kind and shared by the tests below, which leave it unchanged"""
    cfg = H.build_cfg(kind)
    n = _n_icons(kind)
    commands, args, args_dec = H.width_batch(cfg, kind, n, seed=2024)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), WSEED)
    eps = torch.randn(1, 1, n, cfg.dim_z, generator=torch.Generator().manual_seed(2101)) if cfg.use_vae else None
    o_out, o_ld, o_grads = O.loss_and_grads(sd, cfg, commands, args, O.DEFAULT_WEIGHTS, eps=eps, args_dec=args_dec)
    o_out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in o_out.items()}
    o_grads = {k: v for k, v in o_grads.items() if v is not None}
    return cfg, sd, commands, args, args_dec, eps, o_out, {k: v.item() for k, v in o_ld.items()}, o_grads


def _run(kind, dtype, **flags):
    cfg, sd, commands, args, args_dec, eps = _case(kind)[:6]
    model = _hip_model(cfg, sd, dtype).eval()
    for k, v in flags.items():
        setattr(model, k, v)
    return (model,) + _fwd_bwd(model, cfg, commands, args, eps, None, args_dec)


def _logit_keys(o_out):
    return [k for k in ("command_logits", "args_logits", "visibility_logits") if k in o_out]


@pytest.mark.parametrize("kind", KINDS)
def test_fp32_model_matches_oracle_off_the_default_width(gpu_device, kind):
    """the north star's fp32 tolerances (tests/test_model_gpu.py test_fp32_model_matches_oracle_on_fresh_batch), eval mode,
    default work-skipping layouts on"""
    o_out, o_ld, o_grads = _case(kind)[6:]
    model, out, ld, grads = _run(kind, torch.float32)
    worst_l = max((out[k] - o_out[k]).abs().max().item() for k in _logit_keys(o_out))
    worst_loss = max(abs(ld[k] - o_ld[k]) / max(1.0, abs(o_ld[k])) for k in o_ld)
    worst, name = max((H.rel_l2(grads[n], o_grads[n]), n) for n in o_grads)
    print(f"{kind} fp32 vs oracle: worst logit abs err {worst_l:.3e}, worst loss-term rel {worst_loss:.3e}, worst gradient "
          f"rel L2 {worst:.2e} ({name})")
    for k in _logit_keys(o_out):
        assert torch.allclose(out[k], o_out[k], rtol=1e-3, atol=1e-5), (k, (out[k] - o_out[k]).abs().max().item())
    assert torch.equal(out["command_logits"].argmax(-1), o_out["command_logits"].argmax(-1))
    for k in o_ld:
        assert abs(ld[k] - o_ld[k]) <= 1e-4 * max(1.0, abs(o_ld[k])), (k, ld[k], o_ld[k])
    assert worst < 1e-3, f"worst per-tensor gradient relative L2 error {worst:.2e} ({name})"
    if kind == "narrow128_match":
        assert torch.equal(model.last_assignment.long().cpu(), o_out["_assignment"].long())


@pytest.mark.parametrize("kind", ["narrow128", "odd192"])
def test_packed_equals_padded_off_the_default_width(gpu_device, kind):
    """the fp32 assertions of test_packed_encoder_equals_padded_encoder; the packing drops rows"""
    res = {}
    for packed in (True, False):
        model, out, ld, grads = _run(kind, torch.float32, pack_encoder=packed, skip_invisible_backward=packed,
                                     compact_head_backward=packed)
        res[packed] = (out, ld, grads, model.last_packing)
        assert (model.last_live is not None) == packed and (model.last_head_rows is not None) == packed
    total, dense = res[True][3]
    assert res[False][3] is None and 0 < total < dense
    tol = 2e-5
    for k in ("command_logits", "args_logits", "visibility_logits"):
        a, b = res[True][0][k], res[False][0][k]
        assert (a - b).abs().max().item() <= tol * (1.0 + b.abs().max().item()), k
    assert abs(res[True][1]["loss"] - res[False][1]["loss"]) <= tol * abs(res[False][1]["loss"])
    worst, name = max((H.rel_l2(res[True][2][n], res[False][2][n]), n) for n in res[True][2])
    assert worst < 1e-3, f"worst gradient rel L2 {worst:.2e} ({name})"


# bf16 storage / fp32 accumulate against the fp32 oracle, per config:
# (cmd logit abs, args logit abs, cmd argmax agreement, loss rel, grad-norm median rel, grad-norm max rel), then the bounds of
# _check_grad_directions (median, 90th percentile, worst per-tensor relative L2).  Every config starts from the bounds the
# project uses for its default-width cases.  Measured on MI355X (cmd / args / agreement / loss / grad-norm median, max /
# direction median, p90, worst):
#   narrow128        2.9e-2  5.1e-2  0.9976  1.0e-3  2.1e-3  3.8e-2   2.6e-2  7.5e-2  9.1e-2
#   narrow128_vae    3.5e-2  6.6e-2  0.9952  2.6e-3  4.2e-3  6.9e-2   4.7e-2  6.0e-2  8.4e-2
#   narrow128_1s     2.6e-2  3.2e-2  0.9951  2.8e-4  1.4e-3  2.0e-2   1.5e-2  5.4e-2  7.9e-2
#   narrow128_ar     2.3e-2  3.7e-2  0.9755  5.2e-4  1.6e-3  2.5e-2   (see below)
#   narrow128_match  3.1e-2  5.5e-2  0.9856  1.5e-3  3.4e-3  5.9e-2   3.0e-2  1.2e-1  1.6e-1
#   odd192           2.5e-2  4.3e-2  0.9940  6.4e-4  7.7e-4  7.3e-3   1.3e-2  2.3e-2  2.7e-2
#   odd192_1s        2.2e-2  3.8e-2  0.9975  2.9e-4  1.9e-3  2.0e-2   3.4e-2  6.2e-2  7.2e-2
#   odd96            3.0e-2  4.6e-2  0.9928  2.4e-3  1.6e-3  1.1e-2   1.9e-2  5.0e-2  6.8e-2
#   wide512          3.3e-2  3.8e-2  0.9980  6.7e-4  1.3e-3  7.5e-3   2.7e-2  4.5e-2  5.7e-2
#   ff1024           4.3e-2  5.0e-2  0.9995  1.0e-3  1.3e-3  3.6e-3   1.3e-2  1.8e-2  2.4e-2
#   ff1024, mixed    3.0e-2  5.0e-2  1.0000  2.4e-3  4.6e-4  7.2e-3   1.7e-2  2.2e-2  2.5e-2   (fused attention, unfused FFN)
#   nores            2.9e-2  4.8e-2  0.9869  1.2e-3  1.6e-3  4.2e-3   1.5e-2  2.0e-2  2.6e-2
BF16_START = (0.09, 0.10, 0.98, 6e-3, 6e-3, 7e-2)
BF16_WIDTH_BOUNDS = {kind: (BF16_START, BF16_DIR_BOUNDS["default"]) for kind in KINDS}
# Where a config does not meet a starting bound, the bound is not taken from the HIP result but from the yardstick: the oracle on
# the same batch with weights and activations rounded to bf16 (torch.autocast("cpu", torch.bfloat16); tests/bf16_width_yardstick.py
# prints the figures) against the fp32 oracle, times 2 - the project's convention.
# narrow128_ar: 408 command slots whose two best logits often lie within bf16 rounding of each other (51 causal positions x 8
# icons, d_model 128).  The yardstick itself flips 5 of the 408 arg-maxes (agreement 0.9877, deviation 0.0123): bound
# 1 - 2 x 0.0123 = 0.9754.  Its other figures (cmd 2.6e-2, args 3.0e-2, loss 1.0e-3, grad-norm 2.3e-3 / 1.0e-2, direction
# 1.1e-2 / 3.9e-2 / 5.2e-2) lie inside the starting bounds, which stay.  Measured on MI355X: 10 of 408 flipped (0.97549).
BF16_YARDSTICK = {"narrow128_ar": "command arg-max agreement 0.9877 (403 of 408), bound 1 - 2 x (1 - 0.9877) = 0.9754"}
BF16_WIDTH_BOUNDS["narrow128_ar"] = ((0.09, 0.10, 0.9754, 6e-3, 6e-3, 7e-2), BF16_DIR_BOUNDS["default"])


def _check_bf16(what, kind, out, ld, grads):
    o_out, o_ld, o_grads = _case(kind)[6:]
    (b_cl, b_al, b_agree, b_loss, b_gmed, b_gmax), b_dir = BF16_WIDTH_BOUNDS[kind]
    e_c = (out["command_logits"] - o_out["command_logits"]).abs().max().item()
    e_a = (out["args_logits"] - o_out["args_logits"]).abs().max().item()
    agree = (out["command_logits"].argmax(-1) == o_out["command_logits"].argmax(-1)).float().mean().item()
    lrel = max(abs(ld[k] - o_ld[k]) / max(1.0, abs(o_ld[k])) for k in o_ld)
    rel = sorted((abs(grads[n].double().norm().item() - o_grads[n].double().norm().item())
                  / max(o_grads[n].double().norm().item(), 1e-8), n) for n in o_grads)
    _parity_log(f"{what} vs fp32 oracle: command_logits max abs {e_c:.3e} (argmax agree {agree:.4f}), args_logits max abs "
                f"{e_a:.3e}, worst loss-term rel {lrel:.3e}, grad-norm rel median {rel[len(rel) // 2][0]:.3e} max "
                f"{rel[-1][0]:.3e} ({rel[-1][1]})")
    if kind in BF16_YARDSTICK:
        _parity_log(f"{what}: bf16-autocast oracle vs fp32 oracle (the yardstick of the bound): {BF16_YARDSTICK[kind]}")
    assert e_c < b_cl and e_a < b_al and agree > b_agree, (e_c, e_a, agree)
    assert lrel < b_loss, lrel
    assert rel[len(rel) // 2][0] < b_gmed and rel[-1][0] < b_gmax, rel[-1]
    _check_grad_directions(what, grads, o_grads, *b_dir)


@pytest.mark.parametrize("kind", KINDS)
def test_bf16_model_tracks_oracle_off_the_default_width(gpu_device, kind):
    """the quantities of test_bf16_model_tracks_fp32_reference over the oracle's full tensors; the run also shows which
    route the layers took: none of these configurations may reach a fused kernel at its own (small) batch"""
    ops.PROFILE.clear()
    ops.PROFILE_ON = True
    try:
        model, out, ld, grads = _run(kind, torch.bfloat16)
    finally:
        ops.PROFILE_ON = False
    ran = sorted({r[5].get("op") for r in ops.PROFILE if r[5].get("op") in FUSED_OPS})
    ops.PROFILE.clear()
    st = model.store
    if kind in ("narrow128", "odd192", "wide512"):
        assert ran == [] and st._gs is None and st._ffn is None and st._attn is None, (ran, st._gs, st._ffn, st._attn)
    if kind == "ff1024":        # fused attention fits (in_proj 768 x 256), nothing with an FFN inside does
        assert st._attn is not None and st._ffn is None and st._gs is None and ran == []
    _check_bf16(f"bf16 {kind}", kind, out, ld, grads)


def test_mixed_layer_fused_attention_with_unfused_ffn(gpu_device, monkeypatch):
    """ff1024 in bf16 with the row thresholds of the large-stage kernels patched down to this batch: every large layer runs
    the fused attention kernel and the general FFN launches - and still tracks the oracle"""
    monkeypatch.setattr(Fn, "ATTN_MIN_ROWS", 128)
    monkeypatch.setattr(Fn, "FFN_MIN_ROWS", 128)
    ops.PROFILE.clear()
    ops.PROFILE_ON = True
    try:
        model, out, ld, grads = _run("ff1024", torch.bfloat16)
    finally:
        ops.PROFILE_ON = False
    count = lambda name: sum(1 for r in ops.PROFILE if r[5].get("op") == name)        # noqa: E731
    n_attn, n_ffn, n_gs = count("attn_block_fwd"), count("ffn_fwd"), count("gs_layer_fwd") + count("gs_stack_fwd")
    ops.PROFILE.clear()
    assert n_attn > 0 and n_ffn == 0 and n_gs == 0, (n_attn, n_ffn, n_gs)
    _check_bf16("bf16 ff1024 (fused attention, unfused FFN)", "ff1024", out, ld, grads)


@pytest.mark.parametrize("kind", ["narrow128", "odd192", "wide512"])
def test_no_fused_kernel_off_the_default_width_at_any_row_count(gpu_device, monkeypatch, kind):
    """the same with the row thresholds patched down: the shape tests alone keep these widths off the fused kernels"""
    monkeypatch.setattr(Fn, "ATTN_MIN_ROWS", 128)
    monkeypatch.setattr(Fn, "FFN_MIN_ROWS", 128)
    ops.PROFILE.clear()
    ops.PROFILE_ON = True
    try:
        model, out, ld, grads = _run(kind, torch.bfloat16)
    finally:
        ops.PROFILE_ON = False
    ran = sorted({r[5].get("op") for r in ops.PROFILE if r[5].get("op") in FUSED_OPS})
    n_launches = len(ops.PROFILE)
    ops.PROFILE.clear()
    assert n_launches > 0 and ran == [], ran
    o_ld = _case(kind)[7]
    assert abs(ld["loss"] - o_ld["loss"]) <= BF16_WIDTH_BOUNDS[kind][0][3] * abs(o_ld["loss"])


def test_latent_chain_kernel_needs_the_resnet(gpu_device, monkeypatch):
    """use_resnet=False: the one-launch latent chain (ResNet + bottleneck) must not run; with the ResNet, same widths, it does"""
    calls = []
    real = ops.latent_chain_fwd
    monkeypatch.setattr(ops, "latent_chain_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    _run("nores", torch.bfloat16)
    assert calls == []
    commands, args = _case("nores")[2:4]
    cfg = H.build_cfg("nores")
    cfg.use_resnet = True
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), WSEED), torch.bfloat16).eval()
    _fwd_bwd(model, cfg, commands, args)
    assert len(calls) >= 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["narrow128", "odd192"])
def test_training_step_off_the_default_width(gpu_device, kind, dtype):
    """TrainStep for three steps in train mode, eagerly and replayed from the captured graph: finite losses, replay tracks
    eager within the tolerances of test_graph_replay_matches_eager_training, every parameter moved"""
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg(kind)
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 555)
    batches = [H.width_batch(cfg, kind, 8, seed=s)[:2] for s in (11, 12, 11)]
    runs = {}
    for use_graph in (False, True):
        torch.manual_seed(1234)
        model = _hip_model(cfg, sd, dtype).train()
        ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=use_graph)
        losses = [float(ts.step(c.to(DEV), a.to(DEV))["loss"]) for c, a in batches]
        torch.cuda.synchronize()
        assert all(l == l and abs(l) < 1e3 for l in losses), losses
        for n, p in model.named_parameters():
            assert not torch.equal(p.detach().cpu(), sd[n]), f"{n} did not move"
        runs[use_graph] = (losses, model.store.flat.detach().clone(), len(ts._graphs))
    assert runs[True][2] >= 1
    tol = 2e-4 if dtype == torch.float32 else 2e-2
    for a, b in zip(runs[True][0], runs[False][0]):
        assert abs(a - b) <= tol * abs(b), (runs[True][0], runs[False][0])
    d = (runs[True][1] - runs[False][1]).abs()
    assert d.max().item() <= (1.5e-3 if dtype == torch.float32 else 6e-3), \
        f"parameters diverged by {d.max().item():.2e} after 3 steps"
    assert d.mean().item() <= (2e-6 if dtype == torch.float32 else 1e-4), f"mean divergence {d.mean().item():.2e}"
