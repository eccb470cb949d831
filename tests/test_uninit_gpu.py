"""No result may depend on uninitialised memory: whole routes of the model and the geometry modules, run three times - as
they are, with every `torch.empty` / `torch.empty_like` buffer born as NaN, and with it born as 0 (tests/poison.py; integer
buffers are zero in both) - must give the same bits.  The product clears none of its ~200 allocations and its fast paths
skip work (bucketed packed rows, visible groups only, loss-carrying rows only, ld-padded logits, several short sequences per
MFMA tile): every one of them leaves rows, columns or keys a kernel reads but must not use, and a weight-gradient GEMM then
sums over all rows of such a buffer.  Two trainers in one process make the same allocation sequence and get the same stale
blocks back, so test_training_step_is_bit_reproducible cannot see such a dependence; this module can.

Every assertion is exact (`torch.equal`, `==` on floats, `isfinite`).  A failure is narrowed with `poisoned_empty(...,
log=sites)` and `only=` halves of that list (a failing comparison is not a fault: it may be re-run)."""
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import metrics, ops, paths, render
from deepsvg_amd.synthetic import make_batch, make_batch_onestage
from oracle import svg_transformer_oracle as O
from tests import helpers as H
from tests import long_ops_ref as LR
from tests.poison import three_runs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(cfg, sd, dtype, train):
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(sd)
    model.to(DEV)
    model.set_compute_dtype(dtype)
    return model.train(train)


def _same_everywhere(runs, what):
    """runs: [clean, NaN-poisoned, zero-poisoned], each (losses: list of {name: float}, tensors: {name: tensor})"""
    clean = runs[0]
    for losses in clean[0]:
        assert all(v == v and abs(v) < float("inf") for v in losses.values()), (what, losses)
    for name, t in clean[1].items():
        assert t.numel() > 0 and (not t.is_floating_point() or bool(torch.isfinite(t).all())), (what, name)
    for tag, other in zip(("NaN", "zero"), runs[1:]):
        assert other[0] == clean[0], f"{what}: losses under {tag} poison {other[0]} != {clean[0]}"
        assert other[1].keys() == clean[1].keys()
        for name, t in clean[1].items():
            o = other[1][name]
            if not torch.equal(o, t):
                bad = (o != t) | (o != o)
                raise AssertionError(f"{what}: {name} differs under {tag} poison in {int(bad.sum())} of {t.numel()} elements "
                                     f"({int((o != o).sum())} NaN), first at flat index {int(bad.reshape(-1).nonzero()[0])}")


def _train_route(kind, n, *, dtype=torch.bfloat16, use_graph=False, steps=2, dropout=0.1, tweak=None, batch=None, batch2=None,
                 label=False, rel=False, cfg=None, wseed=41, profile=False, lr=1e-3, unordered=()):
    """`steps` TrainStep steps of a fresh model -> (losses of every step, {flat gradient, parameters}).
    unordered: names of parameters whose gradient is summed in a schedule-dependent order (csrc/embed.hip: an argument table
    of more than 288 rows - relative targets - takes the scatter kernel that adds with LDS float atomics inside a workgroup,
    reproducible to ~1e-7 relative and not bit for bit, with or without poison): checked for finiteness, zeroed in the
    gradient that is compared; such a route runs with lr = 0, so that the parameters do not pick the last bits up, and takes
    another batch (batch2) in its second step, which would otherwise repeat the first"""
    from deepsvg_amd.trainer import TrainStep
    cfg = cfg if cfg is not None else H.build_cfg(kind)
    if dropout is not None:
        cfg.dropout = dropout
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), wseed)
    data = []
    for make in [batch if batch is not None else (lambda n_: make_batch(n_, seed=12))] + ([batch2] if batch2 is not None else []):
        c, a = make(n)
        kw = {}
        if label:
            kw["label"] = torch.randint(0, cfg.n_labels, (n,), generator=torch.Generator().manual_seed(1)).to(DEV)
        if rel:
            from oracle import batch_assembly_oracle as B
            r = torch.stack([torch.from_numpy(B.relative_args(c[i, 0].numpy(), a[i, 0].numpy())) for i in range(n)])
            kw["args_dec"] = r.unsqueeze(1).to(DEV)
        data.append((c.to(DEV), a.to(DEV), kw))
    seen = {}

    def run():
        torch.manual_seed(5)
        model = _model(cfg, sd, dtype, True)
        if tweak is not None:
            tweak(model)
        ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=lr, use_graph=use_graph)
        losses = []
        for i in range(steps + (1 if use_graph else 0)):          # graph: capture + `steps` replays
            c, a, kw = data[i % len(data)]
            ld = ts.step(c, a, **kw)
            torch.cuda.synchronize()
            losses.append({k: float(v) for k, v in ld.items()})
        seen["model"] = model
        grad = model.store.grad_buffer(0).detach().clone()
        for name, p in model.named_parameters():
            if name in unordered:
                v = model.store._grad_view(p, 0)
                off = (v.data_ptr() - model.store.grad_buffer(0).data_ptr()) // 4
                assert bool(torch.isfinite(grad[off:off + p.numel()]).all()) and grad[off:off + p.numel()].abs().max() > 0, name
                grad[off:off + p.numel()] = 0
        return losses, {"grad": grad, "params": model.store.flat.detach().clone()}

    runs = three_runs(run)
    if profile:         # which kernels the route reached: a run of its own, compared with nothing.  Under ops.PROFILE_ON the
        # model performs its weight-gradient reductions one by one instead of deferring them (model.py, _runtime: defer is off
        # while profiling), i.e. in another summation order: a profiled step's gradient differs from an unprofiled one's in
        # the last bits, poisoned or not
        ops.PROFILE.clear()
        ops.PROFILE_ON = True
        try:
            run()
        finally:
            ops.PROFILE_ON = False
        seen["ops"] = {r[5].get("op") for r in ops.PROFILE}
        ops.PROFILE.clear()
    return runs, seen


def test_hier_bf16_training_step_eager(gpu_device):
    """320 icons: fused FFN / attention block, ffn_gate_dw2, the LDS-DMA weight-gradient GEMMs, the group-stage stacks, deferred
    reductions, packed encoder, visible-first second stage, compact head rows"""
    runs, seen = _train_route("hier", 320, profile=True)
    assert {"ffn_fwd", "attn_block_fwd", "gs_stack_fwd", "gs_stack_bwd"} <= seen["ops"], sorted(map(str, seen["ops"]))
    m = seen["model"]
    assert m.last_packing is not None and m.last_live is not None and m.last_head_rows is not None
    _same_everywhere(runs, "hier bf16 eager")


def test_hier_bf16_training_step_graph(gpu_device):
    """the same step captured and replayed twice: the static buffers of the captured step (the fills become graph nodes)"""
    runs, seen = _train_route("hier", 320, use_graph=True)
    _same_everywhere(runs, "hier bf16 graph")


def test_hier_bf16_padded_layouts(gpu_device):
    """the reference's padded computation: dense masked layouts in the encoder, every group in the second stage, every row in
    the head"""
    def padded(model):
        model.pack_encoder = model.skip_invisible_backward = model.compact_head_backward = False
    runs, seen = _train_route("hier", 48, tweak=padded)
    m = seen["model"]
    assert m.last_packing is None and m.last_live is None and m.last_head_rows is None
    _same_everywhere(runs, "hier bf16 padded")


def _autograd_route(kind, n, dtype, what, label=False, seed=2024):
    cfg = H.build_cfg(kind)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 777)
    c, a = make_batch(n, seed=seed)
    c, a = c.to(DEV), a.to(DEV)
    lab = torch.randint(0, cfg.n_labels, (n,), generator=torch.Generator().manual_seed(1)).to(DEV) if label else None
    loss_fn = deepsvg_amd.SVGLoss(cfg).to(DEV)

    def run():
        torch.manual_seed(7)
        model = _model(cfg, sd, dtype, False)
        model.zero_grad()
        out = model(c, a, c, a, label=lab, params={})
        ld = loss_fn(out, None, weights=O.DEFAULT_WEIGHTS)
        ld["loss"].backward()
        torch.cuda.synchronize()
        # (the fp32 argument-table scatter adds with LDS float atomics inside a workgroup - csrc/embed.hip, DESIGN.md section 3,
        # the one schedule-dependent sum of the package, exempt in test_full_size_properties_512_icons too: that gradient is
        # checked for finiteness here; test_ignored_inputs_gpu.py pins the kernel's independence from what its tables held
        # with integer-valued gradients, whose sums are exact in any order)
        ts = {"grad:" + k: p.grad.detach().clone() for k, p in model.named_parameters() if not k.endswith("arg_embed.weight")}
        assert all(bool(torch.isfinite(p.grad).all()) for k, p in model.named_parameters() if k.endswith("arg_embed.weight"))
        ts.update({k: out[k].detach().clone() for k in ("command_logits", "args_logits", "visibility_logits")})
        return [{k: float(v.detach()) for k, v in ld.items()}], ts

    runs = three_runs(run)
    assert len(runs[0][1]) > 100
    _same_everywhere(runs, what)


def test_hier_fp32_autograd_forward_loss_backward(gpu_device):
    """the unfused fp32 parity path through autograd: gemm.hip, layernorm.hip, attention.hip, embed.hip, loss.hip; the dense
    logits the model returns are compared too"""
    _autograd_route("hier", 16, torch.float32, "hier fp32 autograd")


def test_fused_argument_head(gpu_device):
    """head_fused.hip: lse / dlogits on the compact token list, logits never stored"""
    import deepsvg_amd.functional as Fn
    saved, lse, dlogits, calls = Fn.HEAD_FUSED, ops.head_lse, ops.head_dlogits, []
    Fn.HEAD_FUSED = True
    ops.head_lse = lambda *a, **k: (calls.append("lse"), lse(*a, **k))[1]
    ops.head_dlogits = lambda *a, **k: (calls.append("dlogits"), dlogits(*a, **k))[1]
    try:
        runs, seen = _train_route("hier", 48)
    finally:
        Fn.HEAD_FUSED, ops.head_lse, ops.head_dlogits = saved, lse, dlogits
    assert calls.count("lse") == 6 and calls.count("dlogits") == 6, calls          # 3 runs x 2 steps
    _same_everywhere(runs, "fused argument head")


@pytest.mark.parametrize("kind", ["onestage", "sketchformer"])
def test_one_stage_routes(gpu_device, kind):
    """50-token sequences in one stage; sketchformer: causal kernels, relative decoder targets"""
    cfg = H.build_cfg(kind)
    rel = kind == "sketchformer"
    runs, _ = _train_route(kind, 32, cfg=cfg, rel=rel, batch=lambda n: make_batch_onestage(n, total_len=cfg.max_total_len, seed=9),
                           batch2=(lambda n: make_batch_onestage(n, total_len=cfg.max_total_len, seed=10)) if rel else None,
                           lr=0.0 if rel else 1e-3, unordered=("decoder.embedding.arg_embed.weight",) if rel else ())
    _same_everywhere(runs, kind)


def test_long_paths_route(gpu_device):
    """max_seq_len = 126: attention_long_mfma.hip, long_seq.hip"""
    runs, _ = _train_route(None, 8, cfg=LR.long_cfg(126), batch=lambda n: make_batch(n, 8, 126, seed=9))
    _same_everywhere(runs, "long paths")


def test_self_matching_route(gpu_device):
    """match.hip: costs, exhaustive assignment, row permutation"""
    runs, seen = _train_route("selfmatch", 32, dropout=None)
    _same_everywhere(runs, "selfmatch")


@pytest.mark.parametrize("kind", ["hier_vae", "fonts"])
def test_vae_and_label_routes(gpu_device, kind):
    """latent_chain_*, the reparametrisation, label embedding (torch.randn_like draws from torch's generator: the same seed)"""
    runs, _ = _train_route(kind, 16, label=kind == "fonts")
    _same_everywhere(runs, kind)


def _same_tensors(runs, what):
    for tag, other in zip(("NaN", "zero"), runs[1:]):
        assert len(other) == len(runs[0])
        for i, (o, t) in enumerate(zip(other, runs[0])):
            assert o.dtype == t.dtype and torch.equal(o, t), f"{what}: output {i} differs under {tag} poison"


def test_greedy_sample_argmax(gpu_device):
    """one-shot decoding at temperature 0: the arg-max head"""
    cfg = H.build_cfg("hier")
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5)
    c, a = (t.to(DEV) for t in make_batch(8, seed=8))

    def run():
        model = _model(cfg, sd, torch.float32, False)
        with torch.no_grad():
            cy, ay = model.greedy_sample(c, a, None, None, concat_groups=False, temperature=0)
        torch.cuda.synchronize()
        return cy.clone(), ay.clone()

    runs = three_runs(run)
    assert runs[0][0].shape == (8, 8, 31) and runs[0][0].unique().numel() > 1
    _same_tensors(runs, "greedy_sample")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("total_len", [40, 70])
def test_autoregressive_sampling_over_the_kv_cache(gpu_device, total_len, dtype):
    """incremental decoding, temperature 0; 70 tokens: the long route, where attention writes the newest row alone (`only_row`)
    into a buffer the caller owns"""
    cfg = H.build_cfg("sketchformer")
    cfg.max_total_len = total_len
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 11)
    sd["decoder.fcn.command_fcn.weight"] = sd["decoder.fcn.command_fcn.weight"] * 8      # spread the command logits
    c, a = (t.to(DEV) for t in make_batch_onestage(16, total_len=total_len, seed=3))

    def run():
        model = _model(cfg, sd, dtype, False)
        model.kv_cache = True
        with torch.no_grad():
            torch.manual_seed(0)
            cy, ay = model._sample_autoregressive(c, a, None, None, 0)
        torch.cuda.synchronize()
        return cy.clone(), ay.clone()

    runs = three_runs(run)
    assert runs[0][0].shape == (16, 1, total_len) and runs[0][0].unique().numel() > 1
    _same_tensors(runs, "autoregressive sampling")


# ---- the geometry modules -------------------------------------------------------------------------------------------------
# Their data-dependent loops (EMD's searches over the arc-length table, the Bezier fit's split / leaf walk and its Ramer-
# Douglas-Peucker twin, the assignment search) have trip counts bounded by integer counts of the input whatever the floats hold:
# a binary search halves an integer interval every round, the fit walk emits a row or splits strictly inside its interval
# (NaN distances end the icon as invalid), the assignment search enumerates a fixed number of maps.  A NaN cannot turn into a hang.
def _nan_aware_equal(o, t):
    if t.is_floating_point():
        return torch.equal(torch.isnan(o), torch.isnan(t)) and torch.equal(torch.nan_to_num(o, nan=0.0), torch.nan_to_num(t, nan=0.0))
    return torch.equal(o, t)


def _same_defined(runs, what):
    """dicts of tensors; NaN is a documented value of some outputs (an empty cloud): it must sit at the same places"""
    for tag, other in zip(("NaN", "zero"), runs[1:]):
        assert other.keys() == runs[0].keys()
        for k, t in runs[0].items():
            assert other[k].dtype == t.dtype and other[k].shape == t.shape and _nan_aware_equal(other[k], t), \
                f"{what}: {k} differs under {tag} poison"


def _float_icons(n, seed):
    c, a = make_batch(n, seed=seed)
    return c.to(DEV), a.float().to(DEV)


@pytest.mark.parametrize("loss", ["chamfer", "emd"])
def test_point_losses_and_their_gradients(gpu_device, loss):
    """chamfer_loss / emd_loss forward and backward, and three steps of metrics.refine(loss=...) on them; the targets are clouds as sample_points
    returns them, rows past the counts poisoned with the rest"""
    c, a = _float_icons(5, 3)
    tc, ta = _float_icons(5, 4)
    tc[1, :, 1:] = 4                                    # an icon with an empty target cloud: per_icon NaN, gradient 0
    fn = metrics.chamfer_loss if loss == "chamfer" else metrics.emd_loss

    def run():
        tp, tn = metrics.sample_points(tc, ta)
        x = a.clone().requires_grad_(True)
        res = fn(c, x, tp, tn)
        res["loss"].backward()
        torch.cuda.synchronize()
        refined, history = metrics.refine(c, a, tp, tn, steps=3, lr=0.1, loss=loss)      # three Adam steps on the same loss
        torch.cuda.synchronize()
        return {"loss": res["loss"].detach(), "per_icon": res["per_icon"].detach(), "valid": res["valid"], "dargs": x.grad.clone(),
                "counts": tn, "refined": refined, "history": history}

    runs = three_runs(run)
    assert bool(torch.isfinite(runs[0]["loss"])) and bool(torch.isfinite(runs[0]["dargs"]).all())
    assert runs[0]["valid"].tolist() == [True, False, True, True, True] and runs[0]["dargs"].abs().sum() > 0
    assert bool(torch.isfinite(runs[0]["history"]).all()) and bool(torch.isfinite(runs[0]["refined"]).all())
    assert not torch.equal(runs[0]["refined"], a)                           # the refinement moved the arguments
    _same_defined(runs, loss)


def test_reconstruction_error(gpu_device):
    g, cfg, commands, args, _ = H.golden_setup("hier_ordered_n5")
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"])
    c, a = commands.to(DEV), args.to(DEV)

    def run():
        res = metrics.reconstruction_error(_model(cfg, sd, torch.float32, False), c, a)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in res.items()}

    runs = three_runs(run)
    re, valid, mean = runs[0]["re"], runs[0]["valid"], runs[0]["mean"]
    assert re.shape == valid.shape == (commands.shape[0],) and torch.equal(torch.isnan(re), ~valid)     # NaN exactly where documented
    assert bool(torch.isfinite(re[valid]).all()) and bool(torch.isfinite(mean)) == bool(valid.any())
    _same_defined(runs, "reconstruction_error")


@pytest.mark.parametrize("fill", [False, True])
def test_rasterize_and_its_gradient(gpu_device, fill):
    c, a = _float_icons(4, 6)
    target = torch.rand(4, 32, 32, generator=torch.Generator().manual_seed(0)).to(DEV)

    def run():
        x = a.clone().requires_grad_(True)
        res = render.image_loss(c, x, target, fill=fill)
        res["loss"].backward()
        torch.cuda.synchronize()
        return {"image": render.rasterize(c, a, size=32, fill=fill), "loss": res["loss"].detach(),
                "per_icon": res["per_icon"].detach(), "dargs": x.grad.clone()}

    runs = three_runs(run)
    assert all(bool(torch.isfinite(v).all()) for v in runs[0].values())
    assert runs[0]["image"].sum() > 0 and runs[0]["dargs"].abs().sum() > 0
    _same_defined(runs, "rasterize")


def test_path_operations(gpu_device):
    """canonicalize, split, simplify: every key of the returned dicts is defined everywhere (padding is EOS / -1 / 0)"""
    c, a = _float_icons(6, 7)

    def run():
        out = {}
        for layout in ("grouped", "concat"):
            r = paths.canonicalize(c, a, layout=layout, max_seq_len=240 if layout == "concat" else None, numericalize=256)
            out.update({f"canon/{layout}/{k}": v for k, v in r.items()})
        s = paths.split(c, a, max_dist=40.0, include_lines=False, max_seq_len=250)
        out.update({f"split/{k}": v for k, v in s.items()})
        f = paths.simplify(s["commands"], s["args"], 0.1, 0.2, 150.0, max_seq_len=250)
        out.update({f"simplify/{k}": v for k, v in f.items()})
        out.update({f"split_n/{k}": v for k, v in paths.split(c, a, n=3, max_seq_len=90).items()})
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}

    runs = three_runs(run)
    for k in ("canon/grouped/valid", "canon/concat/valid", "split/valid", "simplify/valid", "split_n/valid"):
        assert bool(runs[0][k].any()), k                # the check is not vacuous: icons went through
    assert int(runs[0]["split/len_groups"].max()) > int((c != 4).sum(-1).max()) - 1       # rows were added
    _same_defined(runs, "paths")
