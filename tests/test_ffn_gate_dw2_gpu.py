"""ops.ffn_gate_dw2 (csrc/ffn_bwd_gate.hip): dpre and the linear2 weight gradient of the fused FFN backward from one launch,
against the two launches it replaces (the gated GEMM and the split-K weight-gradient GEMM) on the same inputs."""
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_ffn_gate_dw2_has_no_spill_inside_a_loop(tmp_path):
    out = tmp_path / "ffn_bwd_gate.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result",
                    "-Wno-unused-value", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "deepsvg_amd", "csrc", "ffn_bwd_gate.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_loop_mix.py"), "--spills", str(out)],
                       check=True, capture_output=True, text=True)
    rows = [l for l in r.stdout.splitlines() if "scratch instructions" in l]
    inside = [l for l in rows if int(re.search(r"inside loops\s+(\d+)", l).group(1)) > 0]
    assert not inside, "\n".join(inside)
    assert any("mfma" in l for l in r.stdout.splitlines())


def _inputs(T, drop, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dym = (torch.randn(T, 256, generator=g) * 0.5).to(DEV, torch.bfloat16)
    hp = torch.relu(torch.randn(T, 512, generator=g))
    if drop > 0:        # h > 0 <=> ReLU passed AND the hidden dropout kept it
        hp = hp * (torch.rand(T, 512, generator=g) >= drop)
    hp = hp.to(DEV, torch.bfloat16)
    w2p = (torch.randn(256, 512, generator=g) * 0.05).to(DEV, torch.bfloat16)
    return dym, hp, w2p


def _two_launches(dym, hp, w2p, scale, s2):
    from deepsvg_amd import ops
    g2p = torch.empty((256, 512), dtype=torch.float32, device=DEV)
    db2 = torch.empty(256, dtype=torch.float32, device=DEV)
    ops.gemm(dym, hp, a_kc=False, b_kc=False, out=g2p, split_k=s2, rowsum=db2)
    dpre = ops.gemm(dym, w2p, b_kc=False, gate=hp, gate_scale=scale)
    return dpre, g2p, db2


def _one_launch(dym, hp, w2p, scale, s2):
    from deepsvg_amd import ops
    g2p = torch.full((256, 512), float("nan"), dtype=torch.float32, device=DEV)
    db2 = torch.full((256,), float("nan"), dtype=torch.float32, device=DEV)
    dpre = ops.ffn_gate_dw2(dym, hp, w2p, scale, g2p, db2, s2)
    return dpre, g2p, db2


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [4096, 40001, 41216, 63488])
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_ffn_gate_dw2_matches_the_two_launches(gpu_device, T, drop):
    from deepsvg_amd import ops
    dym, hp, w2p = _inputs(T, drop, seed=T + int(drop * 10))
    scale = ops.keep_scale(drop)
    s2 = ops.split_k_for(256, 512, T)
    ref = _two_launches(dym, hp, w2p, scale, s2)
    got = _one_launch(dym, hp, w2p, scale, s2)
    again = _one_launch(dym, hp, w2p, scale, s2)
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]), "dpre differs from the gated GEMM"
    assert torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
    assert _rel_l2(got[1], ref[1]) <= 1e-5, _rel_l2(got[1], ref[1])
    assert _rel_l2(got[2], ref[2]) <= 1e-5, _rel_l2(got[2], ref[2])
    for a, b in zip(got, again):
        assert torch.equal(a, b), "two launches on the same inputs differ"
    # the fp32 master check of the weight gradient itself (not only the two kernels against each other)
    want = dym.float().t() @ hp.float()
    assert _rel_l2(got[1], want) <= 5e-3
    assert _rel_l2(got[2], dym.float().sum(0)) <= 1e-5


@pytest.mark.gpu
def test_ffn_gate_dw2_inside_a_deferral_scope(gpu_device):
    """G2p / db2 are queued like the split-K GEMM's reductions: valid after flush_deferred"""
    from deepsvg_amd import ops
    T = 41216
    dym, hp, w2p = _inputs(T, 0.1, seed=5)
    s2 = ops.split_k_for(256, 512, T)
    ref = _two_launches(dym, hp, w2p, 1.0, s2)
    g2p = torch.empty((256, 512), dtype=torch.float32, device=DEV)
    db2 = torch.empty(256, dtype=torch.float32, device=DEV)
    with ops.DEFER:
        dpre = ops.ffn_gate_dw2(dym, hp, w2p, 1.0, g2p, db2, s2)
    ops.flush_deferred()
    torch.cuda.synchronize()
    assert torch.equal(dpre, ref[0])
    assert _rel_l2(g2p, ref[1]) <= 1e-5 and _rel_l2(db2, ref[2]) <= 1e-5


@pytest.mark.gpu
def test_training_step_with_the_fused_launch(gpu_device, monkeypatch):
    """one bf16 training step (dropout on) from the same weights with DSVG_FFN_GATE_DW2 on and off: the fused route is taken,
    the losses are identical and the flat gradient agrees within fp32 reordering of the linear2 weight-gradient sums"""
    import deepsvg_amd
    from deepsvg_amd import functional, ops
    from deepsvg_amd.trainer import TrainStep
    from tests import helpers as H
    from deepsvg_amd.synthetic import make_batch
    cfg = H.build_cfg("hier")
    cfg.dropout = 0.1
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 77)
    batch = tuple(t.to(DEV) for t in make_batch(640, seed=21))
    calls = []
    fused = ops.ffn_gate_dw2

    def counting(*a, **k):
        calls.append(a[0].shape[0])
        return fused(*a, **k)

    monkeypatch.setattr(ops, "ffn_gate_dw2", counting)
    runs = []
    for on in (False, True):
        monkeypatch.setattr(functional, "FFN_GATE_DW2", on)
        torch.manual_seed(99)
        model = deepsvg_amd.SVGTransformer(cfg)
        model.load_state_dict(sd)
        model.to(DEV)
        model.set_compute_dtype(torch.bfloat16)
        model.train()
        ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(DEV), lr=0.0, use_graph=False)
        losses = {k: float(v) for k, v in ts.step(*batch).items()}
        torch.cuda.synchronize()
        runs.append((losses, model.store.grad_buffer(0).detach().clone()))
    assert calls, "the fused route was not taken"
    assert runs[0][0] == runs[1][0]
    a, b = runs[1][1], runs[0][1]
    assert torch.isfinite(a).all()
    assert _rel_l2(a, b) <= 1e-5
    # everything but the linear2 weight / bias gradients is bit-identical: at most those elements differ
    assert int((a != b).sum()) <= len(calls) * (256 * 512 + 256)
