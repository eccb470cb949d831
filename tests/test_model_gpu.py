"""End-to-end parity of the HIP model on a real MI355X:
  * against the committed golden vectors of the real reference (tests/golden/*.npz),
  * against the oracle on fresh seeded inputs,
at the tolerance BASELINE.json's north_star states for fp32: logits and loss within rtol 1e-3 (atol 1e-5 for
near-zero logits), command-type argmax bit-exact.  bf16 mode is checked at bf16-appropriate tolerances."""
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import ops
from deepsvg_amd.synthetic import make_batch
from oracle import svg_transformer_oracle as O
from tests import helpers as H


pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hip_model(cfg, sd, dtype=torch.float32):
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(sd)
    model.to(DEV)
    model.set_compute_dtype(dtype)
    return model


def _fwd_bwd(model, cfg, commands, args, eps=None, label=None, args_dec=None):
    loss_fn = deepsvg_amd.SVGLoss(cfg).to(DEV)
    model.zero_grad()
    import deepsvg_amd.model as M
    orig = torch.randn_like
    if eps is not None:
        M.torch.randn_like = lambda t: eps.reshape(t.shape).to(device=t.device, dtype=t.dtype)
    try:
        out = model(commands.to(DEV), args.to(DEV), commands.to(DEV), (args if args_dec is None else args_dec).to(DEV),
                    label=label.to(DEV) if label is not None else None, params={})
        ld = loss_fn(out, None, weights=O.DEFAULT_WEIGHTS)
        ld["loss"].backward()
    finally:
        M.torch.randn_like = orig
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}
    out = {k: v.detach().float().cpu() for k, v in out.items() if torch.is_tensor(v)}
    return out, {k: float(v.detach()) for k, v in ld.items()}, grads


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("name", H.golden_cases())
def test_fp32_model_matches_reference_golden(gpu_device, name, packed):
    """packed: first encoder stage on the valid tokens only (default) / on the reference's padded layout"""
    g, cfg, commands, args, eps = H.golden_setup(name)
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"]))
    model.pack_encoder = model.skip_invisible_backward = model.compact_head_backward = packed
    model.eval()
    label = H.golden_label(g)
    out, ld, grads = _fwd_bwd(model, cfg, commands, args, eps, label, H.golden_args_dec(g, args))
    H.check_against_golden(g, out, ld, grads, logit_rtol=1e-3, logit_atol=1e-5, loss_tol=1e-4, grad_norm_rtol=1e-3)
    if "sample_commands" in g:  # autoregressive sampling, the whole batch at once vs the reference's icon-by-icon loop
        cy, ay = model.greedy_sample(commands.to(DEV), args.to(DEV), None, None, concat_groups=False)
        H.check_sampled_sequences(cy, ay, g)
    if "assignment" in g:       # Hungarian self-matching: the assignment the reference's perfect_matching returned
        assert torch.equal(model.last_assignment.long().cpu(), torch.from_numpy(g["assignment"]))
    if eps is None:
        z = model(commands.to(DEV), args.to(DEV), None, None, encode_mode=True).cpu()
        assert torch.allclose(z, torch.from_numpy(g["z"]), rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("name", ["hier_ordered_n5", "fonts_label_n4"])
def test_hierarch_path_matches_reference_golden(gpu_device, name):
    """return_hierarch / hierarch_logits (deepsvg/model/model.py:246-261,379-383): first decoder stage alone against
    the reference's outputs, then fed back into the second stage"""
    g, cfg, commands, args, eps = H.golden_setup(name)
    label = H.golden_label(g)
    label = label.to(DEV) if label is not None else None
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"])).eval()
    import deepsvg_amd.model as M
    orig = torch.randn_like
    if eps is not None:
        M.torch.randn_like = lambda t: eps.reshape(t.shape).to(device=t.device, dtype=t.dtype)
    try:
        with torch.no_grad():
            c, a = commands.to(DEV), args.to(DEV)
            hl, zg = model(c, a, c, a, label=label, return_hierarch=True)
            full = model(c, a, c, a, label=label)
    finally:
        M.torch.randn_like = orig
    assert torch.allclose(hl.cpu(), torch.from_numpy(g["hier_logits"]), rtol=1e-3, atol=1e-5)
    assert torch.allclose(zg.cpu(), torch.from_numpy(g["hier_z"]), rtol=1e-3, atol=1e-5)
    with torch.no_grad():
        again = model(None, None, None, None, label=label, z=zg.permute(2, 1, 0, 3).contiguous(), hierarch_logits=hl,
                      return_tgt=False)
    for k in ("command_logits", "args_logits", "visibility_logits"):
        assert torch.allclose(again[k], full[k], rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_label_conditioned_training_step(gpu_device, dtype):
    """fonts-style config (label_condition, dim_z=128) through TrainStep with dropout on: finite, and the label tables
    and linear_global2 weights move"""
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("fonts")
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 3), dtype).train()
    commands, args = make_batch(16, seed=5)
    label = torch.randint(0, cfg.n_labels, (16,), generator=torch.Generator().manual_seed(1)).to(DEV)
    names = ["encoder.label_embedding.label_embedding.weight", "decoder.label_embedding.label_embedding.weight",
             "encoder.encoder.layers.0.linear_global2.weight", "decoder.decoder.layers.3.linear_global2.weight"]
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n in names}
    assert len(before) == len(names)
    step = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=False)
    commands, args = commands.to(DEV), args.to(DEV)
    losses = [float(step.step(commands, args, label=label)["loss"]) for _ in range(3)]
    assert all(l == l and abs(l) < 1e3 for l in losses), losses
    after = dict(model.named_parameters())
    for n in names:
        assert not torch.equal(before[n], after[n].detach()), n


def test_fp32_model_matches_oracle_on_fresh_batch(gpu_device):
    cfg = H.build_cfg("hier")
    torch.manual_seed(7)
    commands, args = make_batch(24, seed=2024)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 777)
    model = _hip_model(cfg, sd).eval()
    out, ld, grads = _fwd_bwd(model, cfg, commands, args)
    o_out, o_ld, o_grads = O.loss_and_grads(sd, cfg, commands, args)
    for k in ("command_logits", "args_logits", "visibility_logits"):
        assert torch.allclose(out[k], o_out[k].detach(), rtol=1e-3, atol=1e-5), \
            (k, (out[k] - o_out[k].detach()).abs().max().item())
    assert torch.equal(out["command_logits"].argmax(-1), o_out["command_logits"].argmax(-1))
    for k in o_ld:
        assert abs(ld[k] - o_ld[k].item()) <= 1e-4 * max(1.0, abs(o_ld[k].item())), (k, ld[k], o_ld[k].item())
    worst = max(H.rel_l2(grads[n], o_grads[n]) for n in o_grads)
    assert worst < 1e-3, f"worst per-tensor gradient relative L2 error {worst:.2e}"


def test_fp32_model_matches_oracle_at_benchmark_size_512(gpu_device):
    """BASELINE config C2's size (512 icons, hierarchical_ordered) on the fp32 parity path against the CPU oracle
    (~10-20 s of CPU): logits rtol 1e-3 / atol 1e-5, exact command arg-max, losses 1e-4, every parameter gradient
    within 1e-3 relative L2 - the north star's tolerance at the benchmarked shape, default work-skipping layouts on."""
    cfg = H.build_cfg("hier")
    commands, args = make_batch(512, seed=123)              # = bench.py's batch generator
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 99)
    model = _hip_model(cfg, sd).eval()
    out, ld, grads = _fwd_bwd(model, cfg, commands, args)
    assert model.last_packing is not None and model.last_live is not None       # the default (skipping) layouts ran
    o_out, o_ld, o_grads = O.loss_and_grads(sd, cfg, commands, args)
    worst_l = 0.0
    for k in ("command_logits", "args_logits", "visibility_logits"):
        ref = o_out[k].detach()
        err = (out[k] - ref).abs().max().item()
        worst_l = max(worst_l, err)
        assert torch.allclose(out[k], ref, rtol=1e-3, atol=1e-5), (k, err)
    assert torch.equal(out["command_logits"].argmax(-1), o_out["command_logits"].argmax(-1))
    for k in o_ld:
        assert abs(ld[k] - o_ld[k].item()) <= 1e-4 * max(1.0, abs(o_ld[k].item())), (k, ld[k], o_ld[k].item())
    worst, name = max((H.rel_l2(grads[n], o_grads[n]), n) for n in o_grads)
    print(f"N=512 fp32 vs oracle: worst logit abs err {worst_l:.3e}, loss {ld['loss']:.6f} vs {o_ld['loss'].item():.6f}, "
          f"worst gradient rel L2 {worst:.2e} ({name})")
    assert worst < 1e-3, f"worst per-tensor gradient relative L2 error {worst:.2e} ({name})"
    # the same batch on the bf16 throughput path - at this size the fused FFN and fused attention kernels run (>= 16,384
    # rows) - against the same oracle results, with the bounds of the bf16 golden tests; then once more with both fused
    # kernels switched off: the two bf16 paths must agree with each other far better than either does with fp32
    import deepsvg_amd.functional as Fn
    res = {}
    for fused in (True, False):
        saved = (Fn.FFN_MIN_ROWS, Fn.ATTN_MIN_ROWS)
        if not fused:
            Fn.FFN_MIN_ROWS = Fn.ATTN_MIN_ROWS = 1 << 40
        try:
            mb = _hip_model(cfg, sd, torch.bfloat16).eval()
            ops.PROFILE.clear()
            ops.PROFILE_ON = True
            b_out, b_ld, b_grads = _fwd_bwd(mb, cfg, commands, args)
            ops.PROFILE_ON = False
            n_fused = sum(1 for r in ops.PROFILE if r[5].get("op") in ("ffn_fwd", "attn_block_fwd"))
            ops.PROFILE.clear()
        finally:
            ops.PROFILE_ON = False
            Fn.FFN_MIN_ROWS, Fn.ATTN_MIN_ROWS = saved
        # 8 large layers x (FFN, attention), + the second decoder stage's 4 layers once more: the training pass ran the
        # visible groups' sequences, the others run when this test reads the dense logits
        assert (n_fused == 24) if fused else (n_fused == 0), n_fused
        e_c = (b_out["command_logits"].float() - o_out["command_logits"]).abs().max().item()
        e_a = (b_out["args_logits"].float() - o_out["args_logits"]).abs().max().item()
        agree = (b_out["command_logits"].argmax(-1) == o_out["command_logits"].argmax(-1)).float().mean().item()
        lrel = max(abs(b_ld[k] - o_ld[k].item()) / max(1.0, abs(o_ld[k].item())) for k in o_ld)
        rel = sorted(abs(b_grads[n].double().norm().item() - o_grads[n].double().norm().item())
                     / max(o_grads[n].double().norm().item(), 1e-8) for n in o_grads)
        _parity_log(f"N=512 bf16 ({'fused FFN + attention kernels' if fused else 'unfused launches'}) vs fp32 oracle: "
                    f"command_logits max abs {e_c:.3e} (argmax agree {agree:.4f}), args_logits max abs {e_a:.3e}, "
                    f"worst loss-term rel {lrel:.3e}, grad-norm rel median {rel[len(rel) // 2]:.3e} max {rel[-1]:.3e}")
        assert e_c < 0.09 and e_a < 0.12 and agree > 0.98 and lrel < 6e-3
        assert rel[len(rel) // 2] < 6e-3 and rel[-1] < 7e-2
        # direction, not only length: relative L2 distance of EVERY parameter gradient to the oracle's (244 tensors)
        _check_grad_directions(f"N=512 bf16 ({'fused' if fused else 'unfused'})", b_grads, o_grads, *BF16_DIR_BOUNDS["n512"])
        res[fused] = (b_ld["loss"], b_out["command_logits"].float())
    assert abs(res[True][0] - res[False][0]) <= 2e-3 * abs(res[False][0])


@pytest.mark.parametrize("tag", H.sample_cases())
def test_greedy_sample_matches_reference_golden(gpu_device, tag):
    """one-shot greedy_sample on the HIP path (the decode half of BASELINE config C5) against the reference's own
    samples: from the inputs, from z, with forced visibility (one visible group / none), and concat_groups per icon
    (tests/golden/make_golden_sample.py; deepsvg/model/model.py:414-459).  Also temperature=0 (arg-max kernel)."""
    import deepsvg_amd.model as M
    t, cfg = H.sample_fixture(tag)
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), int(t["wseed"]))).eval()
    eps = t.get("eps")
    for temperature in (1e-4, 0):
        def sample(c, a, label, z, hl, concat, icon):
            orig = torch.randn_like
            if eps is not None:
                e = eps if icon is None else eps[:, :, icon:icon + 1]
                M.torch.randn_like = lambda x: e.reshape(x.shape).to(device=x.device, dtype=x.dtype)
            try:
                torch.manual_seed(0)
                return model.greedy_sample(c, a, None, None, label=label, z=z, hierarch_logits=hl, concat_groups=concat,
                                           temperature=temperature)
            finally:
                M.torch.randn_like = orig
        H.run_sample_checks(sample, t, cfg, device=DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_packed_encoder_equals_padded_encoder(gpu_device, dtype):
    """exact padding skip: identical logits / loss / gradients with and without it (to rounding), and the packing
    actually drops rows on the synthetic distribution"""
    cfg = H.build_cfg("hier")
    commands, args = make_batch(40, seed=99)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 321)
    res = {}
    for packed in (True, False):
        model = _hip_model(cfg, sd, dtype).eval()
        model.pack_encoder = model.skip_invisible_backward = model.compact_head_backward = packed
        res[packed] = _fwd_bwd(model, cfg, commands, args) + (model.last_packing,)
        assert (model.last_live is not None) == packed and (model.last_head_rows is not None) == packed
        if packed:
            print(f"decoder stage 2 backward: {model.last_live[0]} of {model.last_live[1]} sequences")
            print(f"argument head backward: {model.last_head_rows[0]} of {model.last_head_rows[1]} tokens")
    total, dense = res[True][3]
    print(f"packed encoder: {total} of {dense} tokens ({100.0 * total / dense:.1f} %)")
    assert res[False][3] is None and 0 < total < 0.6 * dense
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    for k in ("command_logits", "args_logits", "visibility_logits"):
        a, b = res[True][0][k], res[False][0][k]
        assert (a - b).abs().max().item() <= tol * (1.0 + b.abs().max().item()), k
    assert abs(res[True][1]["loss"] - res[False][1]["loss"]) <= tol * abs(res[False][1]["loss"])
    worst, name = max((H.rel_l2(res[True][2][n], res[False][2][n]), n) for n in res[True][2])
    # fp32: the two layouts sum the weight gradients over different token orders / split-K partitions
    assert worst < (1e-3 if dtype == torch.float32 else 6e-2), f"worst gradient rel L2 {worst:.2e} ({name})"


# measured on MI355X (profiles/r02_bf16_parity.log) with a 2x margin; the reference itself under CPU bf16 autocast
# deviates by 1.6e-2 / 2.1e-2 / 9.2e-3 abs on the three logit tensors and flips 0.43 % / 1.5 % of the arg-maxes
BF16_BOUNDS = {
    # name: (cmd logit abs, args logit abs, cmd argmax agreement, loss rel, grad-norm median rel, grad-norm max rel)
    # measured: cmd 4.3e-2 / 3.3e-2 / 2.9e-2 / 4.1e-2, args 2.9e-2 .. 4.7e-2, agreement 0.990 .. 1.0, loss 0.7e-3 .. 3.0e-3,
    # grad-norm median 1.3e-3 .. 2.9e-3, max 1.0e-2 .. 3.5e-2
    "hier_ordered_n2": (0.09, 0.10, 0.98, 6e-3, 6e-3, 7e-2),
    "hier_ordered_n5": (0.09, 0.10, 0.98, 6e-3, 6e-3, 7e-2),
    "onestage50_n3": (0.09, 0.10, 0.98, 6e-3, 6e-3, 7e-2),
    "fonts_label_n4": (0.09, 0.10, 0.98, 6e-3, 6e-3, 7e-2),
}


# per-tensor relative L2 distance of the bf16 path's parameter gradients to the fp32 oracle's: (median, 90th percentile,
# worst) bounds = measured x 2 (profiles/r05_bf16_parity.log)
BF16_DIR_BOUNDS = {
    "default": (0.10, 0.14, 0.22),
    "n512": (2.1e-2, 3.1e-2, 3.5e-2),           # measured 1.04e-2 / 1.52e-2 / 1.72e-2 (fused), 1.00e-2 / 1.40e-2 / 1.56e-2
    "hier_ordered_n2": (5.8e-2, 9.6e-2, 0.15),  # 2.85e-2 / 4.78e-2 / 7.29e-2 (2 icons: few loss rows per gradient)
    "hier_ordered_n5": (4.9e-2, 7.6e-2, 9.3e-2),    # 2.43e-2 / 3.75e-2 / 4.60e-2
    "onestage50_n3": (6.3e-2, 8.3e-2, 0.125),   # 3.14e-2 / 4.14e-2 / 6.09e-2
    "fonts_label_n4": (9.6e-2, 0.14, 0.215),    # 4.80e-2 / 6.86e-2 / 1.06e-1
}


def _check_grad_directions(what, grads, o_grads, b_med, b_p90, b_max):
    rows = sorted((H.rel_l2(grads[n].float().cpu(), o_grads[n]), n) for n in o_grads if o_grads[n] is not None
                  and o_grads[n].double().norm().item() > 0)
    assert len(rows) >= 0.95 * len(o_grads), (len(rows), len(o_grads))
    vals = [r for r, _ in rows]
    med, p90 = vals[len(vals) // 2], vals[int(0.9 * len(vals))]
    _parity_log(f"{what}: gradient direction, rel L2 to the oracle over {len(vals)} tensors: median {med:.3e}, p90 {p90:.3e}, "
                f"worst {vals[-1]:.3e} ({rows[-1][1]}), then {rows[-2][0]:.3e} ({rows[-2][1]}), {rows[-3][0]:.3e} ({rows[-3][1]})")
    assert med < b_med and p90 < b_p90 and vals[-1] < b_max, (what, med, p90, rows[-3:])


def _parity_log(line):
    import os
    print(line)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "bf16_parity.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("name", sorted(BF16_BOUNDS))
def test_bf16_model_tracks_fp32_reference(gpu_device, name):
    """bf16 storage / fp32 accumulate (the throughput path bench.py times) against the fp32 goldens of the REAL
    reference - BASELINE configs C1 (hier_ordered_n2) and C4 (onestage50_n3) included.  Bounds = achieved error x 2."""
    g, cfg, commands, args, eps = H.golden_setup(name)
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"]), torch.bfloat16).eval()
    label = H.golden_label(g)
    out, ld, grads = _fwd_bwd(model, cfg, commands, args, eps, label, H.golden_args_dec(g, args))
    b_cl, b_al, b_agree, b_loss, b_gmed, b_gmax = BF16_BOUNDS[name]
    ref_cl = torch.from_numpy(g["command_logits"])
    err = (out["command_logits"] - ref_cl).abs().max().item()
    agree = (out["command_logits"].argmax(-1) == ref_cl.argmax(-1)).float().mean().item()
    al = out["args_logits"].float().reshape(-1)[::int(g["args_logits_stride"])]
    err_a = (al - torch.from_numpy(g["args_logits_sample"])).abs().max().item()
    agree_a = (out["args_logits"].float().argmax(-1).to(torch.int16) == torch.from_numpy(g["args_argmax"])).float().mean().item()
    names = [str(n) for n in g["grad_names"]]
    rel = [abs(grads[n].double().norm().item() - float(g["grad_norms"][i])) / max(float(g["grad_norms"][i]), 1e-8)
           for i, n in enumerate(names)]
    lrel = max(abs(ld[k] - float(g[k])) / max(1.0, abs(float(g[k])))
               for k in ("loss", "loss_cmd", "loss_args", "loss_visibility", "loss_kl") if k in g and k in ld)
    _parity_log(f"bf16 vs reference fp32 golden {name}: command_logits max abs {err:.3e} (argmax agree {agree:.4f}), "
                f"args_logits sample max abs {err_a:.3e} (argmax agree {agree_a:.4f}), worst loss-term rel {lrel:.3e}, "
                f"grad-norm rel median {sorted(rel)[len(rel) // 2]:.3e} max {max(rel):.3e} ({names[rel.index(max(rel))]})")
    assert err < b_cl and err_a < b_al and agree > b_agree
    assert lrel < b_loss
    assert sorted(rel)[len(rel) // 2] < b_gmed and max(rel) < b_gmax, (max(rel), names[rel.index(max(rel))])
    # direction: the goldens hold norms and samples of the reference's gradients; the full tensors come from the oracle,
    # which tests/test_oracle_golden.py pins to those goldens
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"])
    _, _, o_grads = O.loss_and_grads(sd, cfg, commands, args, O.DEFAULT_WEIGHTS, eps=eps, label=label,
                                     args_dec=H.golden_args_dec(g, args))
    _check_grad_directions(f"bf16 {name}", grads, o_grads, *BF16_DIR_BOUNDS.get(name, BF16_DIR_BOUNDS["default"]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_mode_dropout_step(gpu_device, dtype):
    cfg = H.build_cfg("hier")
    commands, args = make_batch(16, seed=5)
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 3), dtype)
    model.train()
    out1, ld1, g1 = _fwd_bwd(model, cfg, commands, args)
    out2, ld2, g2 = _fwd_bwd(model, cfg, commands, args)
    assert all(torch.isfinite(v).all() for v in g1.values())
    assert ld1["loss"] != ld2["loss"], "dropout masks must change from step to step"
    model.eval()
    _, ld_eval, _ = _fwd_bwd(model, cfg, commands, args)
    assert abs(ld1["loss"] - ld_eval["loss"]) < 1.5 and abs(ld1["loss"] - ld_eval["loss"]) > 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_replay_matches_eager_training(gpu_device, dtype):
    """TrainStep(use_graph=True): one hipGraph per (packed-row bucket, live-sequence bucket), the layout plan computed
    eagerly before each replay.  Three steps on three different batches (same bucket or not) must track the eager
    trainer: same losses, same parameters up to the summation-order differences of the rounded-up row counts."""
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 555)
    batches = [make_batch(48, seed=s) for s in (11, 12, 11)]
    runs = {}
    for use_graph in (False, True):
        torch.manual_seed(1234)
        model = _hip_model(cfg, sd, dtype).train()
        ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=use_graph)
        losses = []
        for c, a in batches:
            ld = ts.step(c.to(DEV), a.to(DEV))
            losses.append(float(ld["loss"]))
        torch.cuda.synchronize()
        runs[use_graph] = (losses, model.store.flat.detach().clone(), len(ts._graphs), model.last_packing)
    assert runs[True][2] >= 1 and runs[True][3] is not None
    tol = 2e-4 if dtype == torch.float32 else 2e-2
    for a, b in zip(runs[True][0], runs[False][0]):
        assert abs(a - b) <= tol * abs(b), (runs[True][0], runs[False][0])
    # Adam moves every weight by ~lr per step whatever the gradient's size, so a rounding-level gradient difference can
    # show up as a fraction of a step on a few weights: bound the worst weight by 1.5 steps and the mean tightly
    d = (runs[True][1] - runs[False][1]).abs()
    # (bf16: rounding-level differences flip more signs; Adam's bias-corrected ratio may exceed 1 in the first steps: ~3-4e-3 worst case)
    # (bf16: 6e-3 = 2 lr x 3 steps, the ceiling of what sign flips of rounding-level gradients can do to one weight)
    assert d.max().item() <= (1.5e-3 if dtype == torch.float32 else 6e-3), \
        f"parameters diverged by {d.max().item():.2e} after 3 steps"
    assert d.mean().item() <= (2e-6 if dtype == torch.float32 else 1e-4), f"mean divergence {d.mean().item():.2e}"


def test_full_size_properties_512_icons(gpu_device):
    """BASELINE config C2 (512 icons, bf16) is too large for the CPU oracle in test time; size-independent properties:
      * determinism: two identical train-mode steps (same seed) give BIT-identical losses and gradients (no atomics in
        any cross-workgroup reduction);
      * the three exact work-skipping layouts change nothing: same loss / logits / gradient norm as the reference's
        padded computation, to bf16 rounding."""
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    commands, args = make_batch(512, seed=123)
    c, a = commands.to(DEV), args.to(DEV)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 99)
    loss_fn = deepsvg_amd.SVGLoss(cfg).to(DEV)

    def run(train, skips, seed=77):
        model = _hip_model(cfg, sd, torch.bfloat16)
        model.pack_encoder = model.skip_invisible_backward = model.compact_head_backward = skips
        model.train(train)
        torch.manual_seed(seed)
        model._seed = None
        model.zero_grad()
        out = model(c, a, c, a, params={})
        ld = loss_fn(out, None, weights=O.DEFAULT_WEIGHTS)
        ld["loss"].backward()
        torch.cuda.synchronize()
        g = model.store.grad_buffer(0).detach().clone()
        run.named = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        return float(ld["loss"].detach()), g, out["command_logits"].detach().float()

    l1, g1, c1 = run(True, True)
    n1 = run.named
    l2, g2, c2 = run(True, True)
    n2 = run.named
    assert l1 == l2 and torch.equal(c1, c2), "train step is not bit-reproducible"
    for n in n1:
        if n.endswith("arg_embed.weight"):
            # the one schedule-dependent sum of the path: LDS float atomics inside a workgroup of the argument-embedding
            # scatter ("Determinism"); everything else reduces in a fixed order
            assert H.rel_l2(n1[n], n2[n]) < 1e-6, n
        else:
            assert torch.equal(n1[n], n2[n]), f"gradient of {n} is not bit-reproducible"
    le, ge, ce = run(False, True)
    lp, gp, cp = run(False, False)
    assert abs(le - lp) <= 2e-3 * abs(lp), (le, lp)
    assert (ce - cp).abs().max().item() <= 3e-2 * (1.0 + cp.abs().max().item())
    assert torch.equal(ce.argmax(-1), cp.argmax(-1)) or (ce.argmax(-1) != cp.argmax(-1)).float().mean().item() < 2e-3
    assert abs(ge.norm().item() - gp.norm().item()) <= 2e-2 * gp.norm().item()
    assert H.rel_l2(ge, gp) < 6e-2


def test_reference_extended_mask_aliasing_on_this_device(gpu_device):
    """Evidence for DESIGN.md: what does the reference's in-place overlapping add (model/utils.py:28) yield on
    torch-ROCm?  (the canonical mask is mask | mask<<3)"""
    pm = torch.zeros(4, 32, device=DEV)
    pm[:, :15] = 1
    canon = torch.zeros_like(pm)
    canon[:, :18] = 1
    torch.narrow(pm, -1, 3, 29).add_(torch.narrow(pm, -1, 0, 29)).clamp_(max=1)
    _parity_log(f"reference-style aliased extended mask on this GPU: {pm[0].int().tolist()}; "
                f"equals canonical (mask | mask << 3): {bool(torch.equal(pm, canon))}")
    # DESIGN.md's claim: on torch-ROCm the overlapping in-place add reads its source before the overlapping writes land
    # (one elementwise kernel, each thread reads both operands first), so the reference computes the canonical mask on
    # a GPU - unlike the CPU loop, whose vectorised chunks feed freshly written values back in (goldens:
    # loss_cmd_ref_aliased).  If this fails the claim is wrong for this torch build and DESIGN.md must say so.
    assert torch.equal(pm, canon)


def test_greedy_sample_and_encode_decode(gpu_device):
    cfg = H.build_cfg("hier")
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5)).eval()
    commands, args = make_batch(4, seed=8)
    z = model(commands.to(DEV), args.to(DEV), None, None, encode_mode=True)
    assert z.shape == (1, 1, 4, 256)
    cy, ay = model.greedy_sample(z=z.permute(2, 1, 0, 3).contiguous(), concat_groups=False)
    assert cy.shape == (4, 8, 31) and ay.shape == (4, 8, 31, 11)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_head_on_the_loss_carrying_slot_range_is_exact(gpu_device, dtype):
    """The argument head + loss run on the argument slots that carry loss somewhere in the batch only (the synthetic and
    the real data have no arcs: slots 0-4 never do).  The skipped slots' logits never enter the loss and their gradients
    are exact zeros: same loss, same gradients as the full 11-slot head; the skipped rows of the head's weight gradient
    are written as zeros."""
    cfg = H.build_cfg("hier")
    commands, args = make_batch(24, seed=31)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 17)
    res = {}
    for on in (True, False):
        model = _hip_model(cfg, sd, dtype).eval()
        model.head_slot_range = on
        out, ld, grads = _fwd_bwd(model, cfg, commands, args)
        res[on] = (ld, grads)
    tol = 1e-5 if dtype == torch.float32 else 3e-3
    for k in res[True][0]:
        assert abs(res[True][0][k] - res[False][0][k]) <= tol * max(1.0, abs(res[False][0][k])), k
    worst, name = max((H.rel_l2(res[True][1][n], res[False][1][n]), n) for n in res[True][1])
    assert worst < (1e-4 if dtype == torch.float32 else 3e-2), (worst, name)
    gw = res[True][1]["decoder.fcn.args_fcn.weight"]
    assert torch.count_nonzero(gw[:5 * 257]) == 0 and torch.count_nonzero(gw[5 * 257:]) > 0


def test_fused_argument_head_and_loss_in_the_model(gpu_device):
    """bf16 training step with the argument head + masked CE on the fused kernels (csrc/head_fused.hip: logits never stored,
    recomputed in the backward pass) against the default head GEMM -> bf16 logits -> masked-CE kernels: the two differ by
    the bf16 rounding of the stored logits only.  With and without the slot-range restriction (6 / 11 slots)."""
    import deepsvg_amd.functional as Fn
    cfg = H.build_cfg("hier")
    commands, args = make_batch(24, seed=33)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 18)
    saved = Fn.HEAD_FUSED
    try:
        for slot_range in (True, False):
            res = {}
            for fused in (True, False):
                Fn.HEAD_FUSED = fused
                model = _hip_model(cfg, sd, torch.bfloat16).eval()
                model.head_slot_range = slot_range
                ops.PROFILE.clear()
                out, ld, grads = _fwd_bwd(model, cfg, commands, args)
                res[fused] = (ld, grads)
            for k in res[True][0]:
                assert abs(res[True][0][k] - res[False][0][k]) <= 2e-3 * max(1.0, abs(res[False][0][k])), k
            worst, name = max((H.rel_l2(res[True][1][n], res[False][1][n]), n) for n in res[True][1])
            assert worst < 3e-2, (worst, name)
    finally:
        Fn.HEAD_FUSED = saved


def test_data_parallel_step_over_rccl_one_rank(gpu_device):
    """The data-parallel TrainStep on a ONE-rank RCCL group (force_ddp): eager (count all-reduce inside the loss, two
    overlapped gradient buckets) and hipGraph mode (count all-reduce before the graph, graph = forward + backward, gradient
    all-reduce + clip + AdamW eagerly behind it - no collective is captured) must both track the plain single-GPU trainer."""
    import os
    import torch.distributed as dist
    from deepsvg_amd.trainer import TrainStep
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{29600 + os.getpid() % 300}", rank=0, world_size=1)
        created = True
    try:
        cfg = H.build_cfg("hier")
        cfg.dropout = 0.1
        sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 321)
        batches = [tuple(t.to(DEV) for t in make_batch(64, seed=s_)) for s_ in (5, 6, 5)]
        runs = {}
        # ddp_bf16 (round 5, DSVG_DDP_BF16): the gradient travels as bf16.  One rank: the collective is an identity, the casts are real
        for name, kw in (("plain", dict(use_graph=True)), ("ddp_graph", dict(use_graph=True, force_ddp=True)),
                         ("ddp_eager", dict(use_graph=False, force_ddp=True)),
                         ("ddp_bf16", dict(use_graph=True, force_ddp=True))):
            torch.manual_seed(7)
            model = _hip_model(cfg, sd, torch.bfloat16).train()
            ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, **kw)
            ts.allreduce_bf16 = name == "ddp_bf16"
            assert ts.ddp == ("force_ddp" in kw)
            losses = [float(ts.step(c, a)["loss"]) for c, a in batches]
            torch.cuda.synchronize()
            runs[name] = (losses, model.store.flat.detach().clone(), ts.grad_norm())
            if name.startswith("ddp_graph"):
                assert len(ts._graphs) >= 1 and ts._counts is not None
        for name in ("ddp_graph", "ddp_eager", "ddp_bf16"):
            for a, b in zip(runs[name][0], runs["plain"][0]):
                assert abs(a - b) <= 2e-2 * abs(b), (name, runs[name][0], runs["plain"][0])
            d = (runs[name][1] - runs["plain"][1]).abs()
            assert d.max().item() <= 6e-3 and d.mean().item() <= 1e-4, (name, d.max().item(), d.mean().item())
            assert abs(runs[name][2] - runs["plain"][2]) <= 5e-2 * runs["plain"][2]
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("use_graph", [False, True])
def test_deferred_gradient_reductions_equal_immediate_ones(gpu_device, dtype, use_graph):
    """TrainStep queues the ~130 partial-sum reductions of the parameter gradients and performs them in a few launches
    after backward (ops.DEFER / flush_deferred); DSVG_DEFER_REDUCE=0 (ts.defer_reductions = False) launches them one by
    one.  Same partial sums, another summation tree: the flat gradient must agree to fp32 rounding, the loss exactly."""
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 77)
    n = 640 if dtype == torch.bfloat16 else 48          # 640 icons: the fused FFN path (>= 16384 rows)
    batches = [tuple(t.to(DEV) for t in make_batch(n, seed=sd_)) for sd_ in (21, 22)]
    runs = {}
    for defer in (False, True):
        torch.manual_seed(99)
        model = _hip_model(cfg, sd, dtype).train()
        ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=0.0, use_graph=use_graph)
        ts.defer_reductions = defer
        for c, a in batches:            # (lr = 0 and two different batches: a stale gradient of step 1 would show)
            ld = ts.step(c, a)
        torch.cuda.synchronize()
        flat = model.store.grad_buffer(0)
        if not use_graph:
            # every parameter's .grad is still the view of the flat buffer the kernels wrote into (no clone on the way)
            for name, p in model.named_parameters():
                assert p.grad is not None and p.grad.data_ptr() == model.store._grad_view(p, 0).data_ptr(), name
        runs[defer] = (float(ld["loss"]), flat.detach().clone(), ts.grad_norm())
    assert runs[True][0] == runs[False][0]
    g1, g0 = runs[True][1], runs[False][1]
    assert torch.isfinite(g1).all() and g0.abs().max().item() > 0
    err = (g1 - g0).abs().max().item()
    assert err <= 3e-6 * g0.abs().max().item() + 1e-9, f"deferred vs immediate gradient: {err:.3e} (max |g| {g0.abs().max().item():.3e})"
    assert abs(runs[True][2] - runs[False][2]) <= 1e-5 * runs[False][2]


def test_training_step_is_bit_reproducible(gpu_device):
    """Two trainers built from the same seed in ONE process, the same two batches (640 icons: every fused kernel runs), dropout
    on: losses and the whole flat gradient are bit-identical - no atomics, no order-dependent reductions, no draw that depends on
    anything but (seed, site, element).  (Round 5: a 64-bit-product form of the dropout word function - v_mad_u64_u32 - broke
    exactly this; the second trainer of a process then differed from the first in the 6th digit of the loss.)"""
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 77)
    batches = [tuple(t.to(DEV) for t in make_batch(640, seed=sd_)) for sd_ in (21, 22)]
    runs = []
    for _ in range(3):
        torch.manual_seed(99)
        model = _hip_model(cfg, sd, torch.bfloat16).train()
        ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=0.0, use_graph=False)
        losses = [{k: float(v) for k, v in ts.step(c, a).items()} for c, a in batches]
        torch.cuda.synchronize()
        runs.append((losses, model.store.grad_buffer(0).detach().clone()))
    for losses, grad in runs[1:]:
        assert losses == runs[0][0]
        assert torch.equal(grad, runs[0][1])


def test_masked_gradient_hand_off_is_taken_and_changes_nothing(gpu_device):
    """functional.LN_BWD_MASKED (round 5): the LayerNorm backward that produces a layer's incoming gradient also writes it with
    the consumer's residual-dropout mask replayed (bit-identical to drop_apply), the consumer takes it by the gradient's address.
    With the switch on the step launches fewer drop_apply kernels and produces bit-identical losses and gradients."""
    import deepsvg_amd.functional as Fn
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 31)
    c, a = (t.to(DEV) for t in make_batch(320, seed=9))
    runs = {}
    saved = Fn.LN_BWD_MASKED
    try:
        for on in (False, True):
            Fn.LN_BWD_MASKED = on
            torch.manual_seed(5)
            model = _hip_model(cfg, sd, torch.bfloat16).train()
            ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=0.0, use_graph=False)
            ops.PROFILE.clear()
            ops.PROFILE_ON = True
            try:
                ld = ts.step(c, a)
                torch.cuda.synchronize()
            finally:
                ops.PROFILE_ON = False
            n_drop = sum(1 for r in ops.PROFILE if r[5].get("op") == "drop_apply")
            ops.PROFILE.clear()
            runs[on] = ({k: float(v) for k, v in ld.items()}, model.store.grad_buffer(0).detach().clone(), n_drop)
    finally:
        Fn.LN_BWD_MASKED = saved
        ops.PROFILE_ON = False
    assert runs[True][0] == runs[False][0] and torch.equal(runs[True][1], runs[False][1])
    assert runs[True][2] <= runs[False][2] - 6, (runs[True][2], runs[False][2])       # 8 large layers: 6+ hand-offs taken


def test_group_stage_stack_launches_in_the_training_step(gpu_device):
    """functional.GS_STACK (round 6): the two group stages (hierarchical_encoder / hierarchical_decoder, 4 layers each) as ONE
    launch per stack and direction (dsvg_gs_stack_fwd / dsvg_gs_stack_bwd) instead of one per layer.  Same arithmetic, same
    stores, same draws, same order of the weight-gradient products: losses AND the flat gradient are bit-identical to the
    per-layer launches, eagerly and replayed from the captured graph; 4 stack launches replace 16 layer launches."""
    import deepsvg_amd.functional as Fn
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 41)
    c, a = (t.to(DEV) for t in make_batch(320, seed=12))
    runs = {}
    saved = Fn.GS_STACK
    try:
        for on in (False, True):
            Fn.GS_STACK = on
            torch.manual_seed(5)
            model = _hip_model(cfg, sd, torch.bfloat16).train()
            ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=0.0, use_graph=False)
            ops.PROFILE.clear()
            ops.PROFILE_ON = True
            try:
                ld = ts.step(c, a)
                torch.cuda.synchronize()
            finally:
                ops.PROFILE_ON = False
            count = lambda name: sum(1 for r in ops.PROFILE if r[5].get("op") == name)
            n = (count("gs_stack_fwd"), count("gs_stack_bwd"), count("gs_layer_fwd"), count("gs_layer_bwd"))
            ops.PROFILE.clear()
            eager = ({k: float(v) for k, v in ld.items()}, model.store.grad_buffer(0).detach().clone())
            # ... and replayed (lr 0: the parameters do not move, the seed advances: compare the two settings step by step)
            torch.manual_seed(5)
            model = _hip_model(cfg, sd, torch.bfloat16).train()
            tg = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=0.0, use_graph=True)
            replay = []
            for _ in range(3):
                ld = tg.step(c, a)
                torch.cuda.synchronize()
                replay.append(({k: float(v) for k, v in ld.items()}, model.store.grad_buffer(0).detach().clone()))
            runs[on] = (eager, n, replay)
    finally:
        Fn.GS_STACK = saved
        ops.PROFILE_ON = False
    assert runs[True][1][:2] == (2, 2) and runs[False][1][:2] == (0, 0), (runs[True][1], runs[False][1])
    assert runs[False][1][2] - runs[True][1][2] == 8 and runs[False][1][3] - runs[True][1][3] == 8      # 2 stacks x 4 layers
    assert runs[True][0][0] == runs[False][0][0]
    assert torch.equal(runs[True][0][1], runs[False][0][1])
    for (la, ga), (lb, gb) in zip(runs[True][2], runs[False][2]):
        assert la == lb and torch.equal(ga, gb)


def test_one_launch_weight_images_equal_the_stand_alone_launches(gpu_device):
    """model.PACK_ONE_LAUNCH (round 5): the bf16 flat copy, the fused FFN / attention / attention-backward / group-stage weight
    images and the seed advance of a training step come from ONE launch (dsvg_pack_images) - bit-identical to the 7 + 1 stand-alone
    launches it replaces, image by image, and in the losses / gradients of two training steps (eager and replayed)."""
    import deepsvg_amd.model as M
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 13)
    batches = [tuple(t.to(DEV) for t in make_batch(320, seed=sd_)) for sd_ in (3, 4)]
    saved = M.PACK_ONE_LAUNCH
    images, runs = {}, {}
    try:
        for on in (False, True):
            M.PACK_ONE_LAUNCH = on
            torch.manual_seed(5)
            model = _hip_model(cfg, sd, torch.bfloat16).train()
            st = model.store
            seed = model.seed_tensor(torch.device(DEV)).clone()
            step = torch.zeros((), dtype=torch.int64, device=DEV)
            st.ensure(torch.device(DEV), torch.bfloat16, advance=(step, seed))
            assert ops.pack_images_ok(st.flat, st.flat_lp) and st._ffn["n"] == 16 and st._attn["n"] == 16 and st._gs["n"] == 12
            assert st._attn["bwd"].numel() == 16 * 128 * 512
            torch.cuda.synchronize()
            images[on] = [t.clone() for t in (st.flat_lp, st._ffn["fwd"], st._ffn["bwd"], st._ffn["b1f"], st._ffn["w2p"],
                                              st._attn["img"], st._attn["bwd"], st._gs["fwd"], st._gs["bwd"], seed, step)]
            for use_graph in (False, True):
                torch.manual_seed(6)
                m2 = _hip_model(cfg, sd, torch.bfloat16).train()
                ts = TrainStep(m2, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=use_graph)
                losses = [{k: float(v) for k, v in ts.step(c, a).items()} for c, a in batches + batches[:1]]
                torch.cuda.synchronize()
                runs[on, use_graph] = (losses, m2.store.flat.detach().clone(), int(ts.step_count))
    finally:
        M.PACK_ONE_LAUNCH = saved
    assert int(images[True][-1]) == 1 and not torch.equal(images[True][-2], model.seed_tensor(torch.device(DEV)))
    for a, b in zip(images[False], images[True]):
        assert a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    for use_graph in (False, True):
        assert runs[True, use_graph][0] == runs[False, use_graph][0]
        assert torch.equal(runs[True, use_graph][1], runs[False, use_graph][1]) and runs[True, use_graph][2] == 3


@pytest.mark.parametrize("use_graph", [False, True])
def test_self_matching_training_step(gpu_device, use_graph):
    """HierarchicalSelfMatching through TrainStep (costs + exhaustive assignment + row permutation have no host round
    trip, so the step is capturable): finite losses, and the assignment is a permutation per icon"""
    from deepsvg_amd.trainer import TrainStep
    cfg = H.build_cfg("selfmatch")
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 3), torch.bfloat16).train()
    commands, args = make_batch(32, seed=9)
    step = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=use_graph)
    commands, args = commands.to(DEV), args.to(DEV)
    losses = [float(step.step(commands, args)["loss"]) for _ in range(3)]
    assert all(l == l and abs(l) < 1e3 for l in losses), losses
    a = model.last_assignment.cpu()
    assert a.shape == (32, cfg.num_groups_proposal)
    assert torch.equal(a.sort(dim=1).values, torch.arange(cfg.num_groups_proposal, dtype=a.dtype).expand_as(a))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_autoregressive_cached_sampling_equals_recompute(gpu_device, dtype):
    """incremental decoding over the per-layer q|k|v cache vs re-running the decoder on the growing prefix (the
    reference's scheme, model.py:428-436): same token sequences; the cached path does T instead of T^2/2 token-layers"""
    import time
    from deepsvg_amd.synthetic import make_batch_onestage
    cfg = H.build_cfg("sketchformer")
    cfg.max_total_len = 40
    model = deepsvg_amd.SVGTransformer(cfg)
    sd = H.weights_for(model, 11)
    sd["decoder.fcn.command_fcn.weight"] = sd["decoder.fcn.command_fcn.weight"] * 8      # spread the command logits
    model = _hip_model(cfg, sd, dtype).eval()
    commands, args = make_batch_onestage(64, total_len=cfg.max_total_len, seed=3)
    commands, args = commands.to(DEV), args.to(DEV)
    outs, secs = {}, {}
    for kv in (True, False):
        model.kv_cache = kv
        with torch.no_grad():
            model._sample_autoregressive(commands[:2], args[:2], None, None, 1e-4)            # warm-up
            torch.cuda.synchronize()
            torch.manual_seed(0)        # the categorical draws (temperature 1e-4: arg-max unless two logits tie within ~1e-3)
            t0 = time.time()
            outs[kv] = model._sample_autoregressive(commands, args, None, None, 1e-4)         # relative args, no cumsum
            torch.cuda.synchronize()
            secs[kv] = time.time() - t0
    print(f"autoregressive sampling, 64 icons x 40 tokens ({dtype}): cached {secs[True] * 1e3:.0f} ms, "
          f"prefix re-computation {secs[False] * 1e3:.0f} ms")
    same_c = (outs[True][0] == outs[False][0]).float().mean().item()
    same_a = (outs[True][1] == outs[False][1]).float().mean().item()
    # same recurrence, same draws: identical up to near-ties (a flipped token also changes what follows it)
    lo = 0.995 if dtype == torch.float32 else 0.9
    assert same_c >= lo and same_a >= lo, (same_c, same_a)
    assert outs[True][0].unique().numel() > 1


def test_greedy_sample_temperature_zero_is_the_argmax(gpu_device):
    """temperature = 0 (arg-max kernel on the stored logits) against the reference's temperature 1e-4 draw"""
    cfg = H.build_cfg("hier")
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5)).eval()
    commands, args = make_batch(8, seed=8)
    z = model(commands.to(DEV), args.to(DEV), None, None, encode_mode=True).permute(2, 1, 0, 3).contiguous()
    a = model.greedy_sample(z=z, concat_groups=False, temperature=0)
    torch.manual_seed(0)
    b = model.greedy_sample(z=z, concat_groups=False)
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    assert (a[0] == b[0]).float().mean().item() > 0.999 and (a[1] == b[1]).float().mean().item() > 0.999


@pytest.mark.parametrize("use_graph", [False, True])
def test_autoregressive_training_step(gpu_device, use_graph):
    """Sketchformer-style config (teacher forcing through the causal kernels, relative decoder targets) through
    TrainStep: the loss goes down on a fixed batch"""
    from deepsvg_amd.synthetic import make_batch_onestage
    from deepsvg_amd.trainer import TrainStep
    from oracle import batch_assembly_oracle as B
    cfg = H.build_cfg("sketchformer")
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 3), torch.bfloat16).train()
    commands, args = make_batch_onestage(32, total_len=cfg.max_total_len, seed=9)
    rel = torch.stack([torch.from_numpy(B.relative_args(commands[i, 0].numpy(), args[i, 0].numpy())) for i in range(32)])
    args_rel = rel.unsqueeze(1)
    step = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=use_graph)
    commands, args, args_rel = commands.to(DEV), args.to(DEV), args_rel.to(DEV)
    losses = [float(step.step(commands, args, args_dec=args_rel)["loss"]) for _ in range(12)]
    assert all(l == l and abs(l) < 1e3 for l in losses), losses
    assert sum(losses[-3:]) < sum(losses[:3]), losses


def test_self_matching_full_size_properties(gpu_device):
    """BASELINE's batch (512 icons): the assignment is a permutation per icon and - being the exact minimum - costs no
    more than the identity pairing or any random pairing of the visible targets"""
    from deepsvg_amd import ops
    from deepsvg_amd.svgtensor import CMD_ARGS_MASK
    cfg = H.build_cfg("selfmatch")
    model = _hip_model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 2), torch.bfloat16).eval()
    commands, args = make_batch(512, seed=12)
    c, a = commands.to(DEV), args.to(DEV)
    with torch.no_grad():
        plain = model(c, a, c, a, return_tgt=False)                         # predictions in their own order
        G = cfg.num_groups_proposal
        S = c.shape[-1] - 1
        cl = plain["command_logits"].reshape(512 * G * S, -1)
        al = plain["args_logits"].reshape(512 * G * S, -1)
        vl = plain["visibility_logits"].reshape(512 * G, 2)
        cost, vis = ops.match_costs(cl, al, vl, c, a, CMD_ARGS_MASK.float().to(DEV), 512, G, G, cfg.n_args,
                                    model.args_dim, cfg.n_commands, 4)
        assign, idx, inv = ops.match_assign(cost, vis)
        matched = model(c, a, c, a)                                         # train-mode call: matched order
    assert torch.equal(model.last_assignment, assign)
    assert torch.equal(assign.sort(dim=1).values, torch.arange(G, device=DEV, dtype=assign.dtype).expand(512, G))
    assert torch.equal(idx[inv.long()], torch.arange(512 * G, device=DEV, dtype=idx.dtype))
    # output slot j carries prediction assign[j]
    want = plain["command_logits"].gather(1, assign.long().view(512, G, 1, 1).expand_as(plain["command_logits"]))
    assert torch.equal(matched["command_logits"], want)
    # optimality: total cost of the visible targets under the assignment <= identity and <= random pairings
    cost = torch.nan_to_num(cost, nan=0.0)
    n_vis = vis.sum(1)
    rank = (vis.cumsum(1) - 1).clamp_min(0).long()                          # j-th visible target -> slot j
    picked = assign.long().gather(1, rank)                                  # prediction matched to target g
    tot = (cost.gather(2, picked.unsqueeze(-1)).squeeze(-1) * vis).sum(1)
    ident = (cost.diagonal(dim1=1, dim2=2) * vis).sum(1)
    assert bool((tot <= ident + 1e-4).all())
    gen = torch.Generator().manual_seed(0)
    for _ in range(4):
        perm = torch.stack([torch.randperm(G, generator=gen) for _ in range(512)]).to(DEV)
        rnd = (cost.gather(2, perm.unsqueeze(-1)).squeeze(-1) * vis).sum(1)
        assert bool((tot <= rnd + 1e-4).all())
    assert int(n_vis.min()) >= 1
