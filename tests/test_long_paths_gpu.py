"""Two-stage configs with paths of 65..256 tokens on the GPU: the new kernels (build_masks_lens, pack_tokens_lens, the packed
mean-pool, the packed VALU long attention and the bf16 matrix-core long attention of csrc/attention_long_mfma.hip) against
plain-torch restatements, and the model against the reference golden and the oracle."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import deepsvg_amd
from oracle import svg_transformer_oracle as O
from tests import helpers as H
from tests import long_ops_ref as LR
from tests import torch_ops_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GOLDEN = os.path.join(H.GOLDEN_DIR, "long", "hier_long100_n3.npz")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_long_mfma_kernel_isa(tmp_path):
    out = tmp_path / "attention_long_mfma.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result",
                    "-Wno-unused-value", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "deepsvg_amd", "csrc", "attention_long_mfma.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_loop_mix.py"), "--spills", str(out)],
                       check=True, capture_output=True, text=True)
    assert "scratch instructions" not in r.stdout, r.stdout
    code = [l.split(";")[0].strip() for l in out.read_text().splitlines()]
    ops_ = [l.split()[0] for l in code if l and not l.startswith(".") and not l.endswith(":")]
    assert sum(o.startswith("v_mfma_f32_32x32x16_bf16") for o in ops_) >= 40
    assert not [o for o in ops_ if o.startswith(("flat_", "scratch_"))]


def _lens_cases(n, S, g):
    lens = torch.randint(0, S + 1, (n,), generator=g)
    lens[:4] = torch.tensor([0, 1, S - 1, S])
    return lens.to(torch.int32)


def _commands(lens, S, g):
    """commands [n, S] whose first EOS (4) sits at lens[b], with extra EOS tokens at random places behind it"""
    n = lens.numel()
    c = torch.randint(0, 4, (n, S), generator=g).float()
    pos = torch.arange(S).unsqueeze(0)
    c[pos == lens.long().unsqueeze(1)] = 4.0
    extra = (torch.rand(n, S, generator=g) < 0.5) & (pos > lens.long().unsqueeze(1))
    c[extra] = 4.0
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("S", [65, 102, 256])
def test_masks_packing_pooling_match_restatements(S):
    from deepsvg_amd import ops
    g = torch.Generator().manual_seed(S)
    G, n = 8, 64
    lens = _lens_cases(n, S, g)
    cmd = _commands(lens, S, g)
    cmd[5] = 4.0                                    # all-EOS row: invisible
    args = torch.randint(-1, 256, (n * S, 11), generator=g).float()
    got = ops.build_masks_lens(cmd.to(DEV), S, G, 4, want_group_mask=True)
    want = LR.build_masks_lens(cmd, S, G, 4, want_group_mask=True)
    for x, y in zip(got, want):
        assert torch.equal(x.cpu(), y)
    assert torch.equal(got[0].cpu(), ops.seq_lens(cmd.to(DEV), S).cpu())
    gp = ops.pack_tokens_lens(cmd.to(DEV).view(-1), args.to(DEV), got[0], n, S)
    wp = LR.pack_tokens_lens(cmd.view(-1), args, want[0], n, S)
    for x, y in zip(gp, wp):
        assert torch.equal(x.cpu(), y)
    seq_off = gp[0]
    total = int(seq_off[-1])
    rows = min((total + 127) // 128 * 128, n * S)
    nz = want[0] > 0
    off = seq_off.cpu().long()
    inv = (1.0 / want[0].float())                   # fp32, as the kernels: sum in row order, times 1 / len
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(rows, 256, generator=g).to(DEV, dt)
        m = ops.masked_mean_fwd(x, None, n, S, seq_off=seq_off).cpu()
        xc = x.cpu().float()
        wm = torch.zeros(n, 256)
        for b in range(n):
            acc = torch.zeros(256)
            for i in range(int(off[b]), int(off[b + 1])):
                acc = acc + xc[i]
            wm[b] = acc * inv[b]
        assert torch.equal(m[nz], wm.to(dt)[nz]) and torch.isnan(m[~nz].float()).all()
        dout = torch.randn(n, 256, generator=g).to(DEV, dt)
        dx = ops.masked_mean_bwd(dout, None, n, S, seq_off=seq_off, total_rows=rows).cpu()
        rowg = (dout.cpu().float() * inv.unsqueeze(1)).to(dt)
        seq_of_row = torch.repeat_interleave(torch.arange(n), (off[1:] - off[:-1]))
        assert torch.equal(dx[:total], rowg[seq_of_row]) and (dx[total:] == 0).all()
        # the padded layout pools through dsvg_prefix_mean (unchanged) with the same lengths
        xd = torch.randn(n * S, 256, generator=g).to(DEV, dt)
        pd = ops.masked_mean_fwd(xd, got[0], n, S).cpu()
        pk = ops.masked_mean_fwd(_pack(xd, got[0], S), None, n, S, seq_off=seq_off).cpu()
        assert torch.equal(pd[nz], pk[nz])


def _attn_inputs(n, S, H_, g, dt):
    lens = _lens_cases(n, S, g)
    qkv = (torch.randn(n * S, 3 * 32 * H_, generator=g) * 0.7).to(DEV, dt)
    dout = torch.randn(n * S, 32 * H_, generator=g).to(DEV, dt)
    seq_off = torch.zeros(n + 1, dtype=torch.int32)
    seq_off[1:] = torch.cumsum(lens.long(), 0).to(torch.int32)
    return lens.to(DEV), qkv, dout, seq_off.to(DEV)


def _pack(x, lens, S):
    n = lens.numel()
    valid = (torch.arange(S, device=x.device).unsqueeze(0) < lens.long().unsqueeze(1)).reshape(-1)
    return x[valid].contiguous()


def _unpack(xp, lens, S, rows):
    n = lens.numel()
    valid = (torch.arange(S, device=xp.device).unsqueeze(0) < lens.long().unsqueeze(1)).reshape(-1)
    out = torch.zeros((n * S, xp.shape[1]), dtype=xp.dtype, device=xp.device)
    out[valid] = xp[:int(valid.sum())]
    return out


def _rel(a, b, mask=None):
    a, b = a.double(), b.double()
    if mask is not None:
        a, b = a[mask], b[mask]
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


SEED = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("S,H_", [(65, 8), (66, 1), (96, 2), (101, 8), (102, 8), (128, 4), (200, 8), (256, 8)])
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_long_attention_kernels_match_restatement(S, H_, drop):
    from deepsvg_amd import ops
    g = torch.Generator().manual_seed(S * 16 + H_)
    n = 24
    scale = 32 ** -0.5
    seed = SEED.to(DEV)
    for dt, tol in ((torch.float32, 2e-5), (torch.bfloat16, 2.5e-2)):
        lens, qkv, dout, seq_off = _attn_inputs(n, S, H_, g, dt)
        # (a sequence without keys: NaN in the restatement's softmax, zeros from every kernel)
        want = ref.attention_fwd(qkv.cpu(), lens.cpu(), n, S, H_, scale, drop, 7, SEED).float().nan_to_num(0.0)
        wd = ref.attention_bwd(qkv.cpu(), lens.cpu(), dout.cpu(), n, S, H_, scale, drop, 7, SEED).float().nan_to_num(0.0)
        vq = (torch.arange(S).unsqueeze(0) < lens.cpu().long().unsqueeze(1)).reshape(-1)   # rows of valid tokens
        # padded (the path-stage route: bf16 -> matrix cores, fp32 -> the VALU long kernels)
        o = ops.attention_fwd(qkv, lens, n, S, H_, scale, drop, 7, seed, path_stage=True).float().cpu()
        d = ops.attention_bwd(qkv, lens, dout, n, S, H_, scale, drop, 7, seed, path_stage=True).float().cpu()
        assert _rel(o, want) < tol and _rel(d, wd) < tol, (dt, _rel(o, want), _rel(d, wd))
        # packed (valid rows only + 40 pad rows), compared on the valid rows; pad rows zero-filled.  The packed layout has
        # no query rows past a length: against the padded layout whose such rows carry a zero output gradient
        dout = dout * vq.to(DEV).unsqueeze(1).to(dt)
        wd = ref.attention_bwd(qkv.cpu(), lens.cpu(), dout.cpu(), n, S, H_, scale, drop, 7, SEED).float().nan_to_num(0.0)
        d = ops.attention_bwd(qkv, lens, dout, n, S, H_, scale, drop, 7, seed, path_stage=True).float().cpu()
        qp = torch.cat([_pack(qkv, lens, S), torch.full((40, qkv.shape[1]), 3.0, dtype=dt, device=DEV)])
        dp_ = torch.cat([_pack(dout, lens, S), torch.full((40, dout.shape[1]), 3.0, dtype=dt, device=DEV)])
        op = ops.attention_fwd(qp, None, n, S, H_, scale, drop, 7, seed, seq_off=seq_off)
        dpk = ops.attention_bwd(qp, None, dp_, n, S, H_, scale, drop, 7, seed, seq_off=seq_off)
        tot = int(seq_off[-1])
        assert (op[tot:] == 0).all() and (dpk[tot:] == 0).all()
        op_d = _unpack(op, lens, S, qp.shape[0]).float().cpu()
        dpk_d = _unpack(dpk, lens, S, qp.shape[0]).float().cpu()
        assert _rel(op_d, want, vq) < tol and _rel(dpk_d, wd, vq) < tol
        # packed and padded agree on the valid rows (same kernel family, same draws)
        assert _rel(op_d, o, vq) < tol and _rel(dpk_d, d, vq) < tol
        if dt == torch.bfloat16 and drop > 0:
            # the matrix-core kernels draw the VALU long kernels' dropout mask: same inputs, p = 0.1, both routes
            ov = ops.attention_fwd(qkv, lens, n, S, H_, scale, drop, 7, seed).float().cpu()      # one-stage route: VALU
            assert _rel(o, ov) < 2e-2


def _model(cfg, sd, dtype=torch.float32, pack=True):
    m = deepsvg_amd.SVGTransformer(cfg)
    m.load_state_dict(sd)
    m.pack_encoder = pack
    return m.to(DEV).set_compute_dtype(dtype)


def _loss_grads(model, cfg, c, a, label=None):
    model.eval()
    model.zero_grad()
    out = model(c.to(DEV), a.to(DEV), c.to(DEV), a.to(DEV), label=None if label is None else label.to(DEV), params={})
    ld = deepsvg_amd.SVGLoss(cfg).to(DEV)(out, None, weights=O.DEFAULT_WEIGHTS)
    ld["loss"].backward()
    torch.cuda.synchronize()
    out = {k: v.detach().float().cpu() for k, v in out.items() if torch.is_tensor(v)}
    grads = {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}
    return out, {k: v.item() for k, v in ld.items()}, grads


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [True, False])
def test_long_path_model_matches_reference_golden(pack):
    g = dict(np.load(GOLDEN, allow_pickle=False))
    cfg = LR.long_cfg(100)
    c, a = torch.from_numpy(g["commands"]), torch.from_numpy(g["args"])
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"])
    model = _model(cfg, sd, pack=pack)
    out, ld, grads = _loss_grads(model, cfg, c, a)
    assert (model.last_packing is not None) == pack
    H.check_against_golden(g, out, ld, grads, logit_rtol=1e-3, logit_atol=1e-5, loss_tol=1e-4, grad_norm_rtol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("L,kind", [(63, "hier"), (126, "hier"), (126, "fonts")])
def test_long_path_model_matches_oracle(L, kind):
    from deepsvg_amd.synthetic import make_batch
    cfg = LR.long_cfg(L, kind)
    c, a = make_batch(4, 8, L, seed=L)
    label = torch.tensor([3, 17, 42, 99]) if cfg.label_condition else None
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 77)
    out, ld, grads = _loss_grads(_model(cfg, sd), cfg, c, a, label)
    o_out, o_ld, o_grads = O.loss_and_grads(sd, cfg, c, a, O.DEFAULT_WEIGHTS, label=label)
    cl, ocl = out["command_logits"], o_out["command_logits"].detach()
    assert torch.allclose(cl, ocl, rtol=1e-3, atol=1e-5), (cl - ocl).abs().max().item()
    assert torch.equal(cl.argmax(-1), ocl.argmax(-1))
    assert abs(ld["loss"] - o_ld["loss"].item()) <= 1e-4 * abs(o_ld["loss"].item())
    worst = max(H.rel_l2(grads[n], o_grads[n]) for n in grads)
    assert worst < 1e-3, worst


# measured error x 2 (profiles/long_paths_bf16_bounds.log)
BF16_LONG_BOUNDS = dict(argmax=0.9992, grad_dir=5.7e-3)


@pytest.mark.gpu
def test_long_path_bf16_model_tracks_fp32():
    from deepsvg_amd.synthetic import make_batch
    cfg = LR.long_cfg(100)
    c, a = make_batch(16, 8, 100, seed=3)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5)
    o32, _, g32 = _loss_grads(_model(cfg, sd), cfg, c, a)
    o16, _, g16 = _loss_grads(_model(cfg, sd, torch.bfloat16), cfg, c, a)
    agree = (o16["command_logits"].argmax(-1) == o32["command_logits"].argmax(-1)).float().mean().item()
    worst = max(1 - torch.nn.functional.cosine_similarity(g16[n].reshape(1, -1).double(), g32[n].reshape(1, -1).double()).item()
                for n in g32 if g32[n].norm() > 0)
    print(f"bf16 vs fp32, max_seq_len 100, 16 icons: command argmax agreement {agree:.5f}, worst gradient 1 - cos {worst:.3e}")
    assert agree >= BF16_LONG_BOUNDS["argmax"] and worst <= BF16_LONG_BOUNDS["grad_dir"], (agree, worst)


@pytest.mark.gpu
def test_long_path_training_step_graph_matches_eager_and_repeats():
    """bf16 TrainStep of a max_seq_len = 100 config: the hipGraph replay tracks the eager step (up to the summation-order
    differences of its rounded-up row buckets, the bounds of test_model_gpu.py::test_graph_replay_matches_eager_training),
    and two trainers from one seed give bit-identical losses and parameters (= flat gradients), eager and replayed"""
    from deepsvg_amd.synthetic import make_batch
    from deepsvg_amd.trainer import TrainStep
    cfg = LR.long_cfg(100)
    cfg.dropout = 0.1
    batches = [make_batch(8, 8, 100, seed=s) for s in (9, 10, 9)]
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5)

    def run(graph):
        torch.manual_seed(0)
        m = _model(cfg, sd, torch.bfloat16)
        m.train()
        ts = TrainStep(m, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=1e-3, use_graph=graph)
        losses = [ts.step(c.to(DEV), a.to(DEV))["loss"].item() for c, a in batches]
        torch.cuda.synchronize()
        return losses, m.store.flat.detach().clone().cpu()

    l_e, p_e = run(False)
    l_e2, p_e2 = run(False)
    l_g, p_g = run(True)
    l_g2, p_g2 = run(True)
    assert l_e == l_e2 and torch.equal(p_e, p_e2)
    assert l_g == l_g2 and torch.equal(p_g, p_g2)
    for x, y in zip(l_g, l_e):
        assert abs(x - y) <= 2e-2 * abs(y), (l_g, l_e)
    d = (p_g - p_e).abs()
    assert d.max().item() <= 6e-3 and d.mean().item() <= 1e-4, (d.max().item(), d.mean().item())


@pytest.mark.gpu
def test_long_path_greedy_sample_matches_oracle():
    from deepsvg_amd.synthetic import make_batch
    cfg = LR.long_cfg(100)
    c, a = make_batch(3, 8, 100, seed=11)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5)
    m = _model(cfg, sd).eval()
    with torch.no_grad():
        cy, ay = m.greedy_sample(c.to(DEV), a.to(DEV), None, None, concat_groups=False)
    want, _wa, gap, _ag = O.greedy_sample(sd, cfg, c, a, concat_groups=False)
    assert cy.shape == want.shape
    clear = gap > 1e-3          # (the reference's draw at temperature 1e-4 is the arg-max away from near-ties)
    assert clear.float().mean() > 0.9 and torch.equal(cy.cpu()[clear], want[clear])


@pytest.mark.gpu
def test_default_config_calls_no_new_entry_point(monkeypatch):
    """max_seq_len = 30: a training step reaches none of the ops added for long paths"""
    from deepsvg_amd import ops, lib
    from deepsvg_amd.synthetic import make_batch
    from deepsvg_amd.trainer import TrainStep
    called = []
    L = lib.load()
    new = ("dsvg_build_masks_lens", "dsvg_pack_tokens_lens", "dsvg_packed_mean_fwd", "dsvg_packed_mean_bwd",
           "dsvg_attention_long_packed_fwd", "dsvg_attention_long_packed_bwd", "dsvg_attention_long_mfma_fwd",
           "dsvg_attention_long_mfma_bwd")

    class Spy:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            if name in new:
                called.append(name)
            return getattr(self._real, name)

    monkeypatch.setattr(ops._l, "load", lambda: Spy(L))
    for name in ("build_masks_lens", "pack_tokens_lens"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a_, _r=real, _n=name, **k: (called.append(_n), _r(*a_, **k))[1])
    cfg = LR.long_cfg(30)
    c, a = make_batch(8, seed=1)
    m = _model(cfg, H.weights_for(deepsvg_amd.SVGTransformer(cfg), 5), torch.bfloat16)
    m.train()
    ts = TrainStep(m, deepsvg_amd.SVGLoss(cfg).to(DEV))
    ts.step(c.to(DEV), a.to(DEV))
    torch.cuda.synchronize()
    assert not called, called
