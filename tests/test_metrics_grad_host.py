"""The gradient of deepsvg_amd.metrics on CPU: the float64 restatements of the three backward ops
(tests/metrics_grad_ref.py) against the reference's own autograd (tests/golden/metrics/metrics_grad.npz,
make_golden_metrics_grad.py), and the autograd wiring of sample_points / chamfer / chamfer_loss / refine with the ops
replaced by restatements.

Bound: 4 x `ref_spread`, the fixture's own measure of what the reference's fp32 sampling costs its gradient (the largest
difference between the reference's gradient and the float64 restatement's when the fixture was made)."""
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import metrics
from tests import helpers as H
from tests import metrics_grad_ref as GR
from tests import metrics_ref as MR
from tests.test_metrics_host import CHAMFER_ATOL, golden

GOLDEN_GRAD = os.path.join(H.GOLDEN_DIR, "metrics", "metrics_grad.npz")
N = 10


@pytest.fixture
def metric_grad_ops(emulated_ops):
    saved = GR.install()
    yield
    GR.restore(saved)


def golden_grad():
    """-> fixture dict, commands [12, 66], jittered args [12, 66, 11], pairs [6, 2] (long)"""
    base, commands, _ = golden()
    g = dict(np.load(GOLDEN_GRAD, allow_pickle=False))
    return g, commands, torch.from_numpy(g["args"]), torch.from_numpy(base["pairs"]).long()


def grad_bound(g):
    return 4.0 * float(g["ref_spread"])


def test_fixture_margins():
    g, _, args, _ = golden_grad()
    assert float(g["min_gap"]) >= 1e-3 and float(g["min_dist"]) >= 1e-2 and 0 < float(g["ref_spread"]) < 2e-6
    assert args.dtype == torch.float32 and not bool(torch.isnan(torch.from_numpy(g["grad_x"])).any())


def test_restated_gradient_matches_the_reference():
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    px, nx = MR.sample_points(commands[i], args[i], N)                  # fp32 points, as the kernel's
    py, ny = MR.sample_points(commands[j], args[j], N)
    out, idx_x, idx_y = GR.chamfer_nn(px, nx, py, ny)
    dpx, dpy = GR.chamfer_bwd(px, nx, py, ny, idx_x, idx_y, torch.ones(len(pairs)), as_double=True)
    gx = GR.sample_points_bwd(commands[i], dpx.float(), N, as_double=True)
    gy = GR.sample_points_bwd(commands[j], dpy.float(), N, as_double=True)
    err = max((gx - torch.from_numpy(g["grad_x"])).abs().max().item(), (gy - torch.from_numpy(g["grad_y"])).abs().max().item())
    print(f"restated gradient vs the reference's autograd: max abs err {err:.3e} (bound {grad_bound(g):.3e})")
    assert err <= grad_bound(g)
    assert (out.double() - torch.from_numpy(g["loss"])).abs().max().item() <= CHAMFER_ATOL


def test_restated_sample_points_bwd_is_the_transpose_of_the_forward():
    """autograd through the forward restatement (an independent statement of the weights and of the start-point rule)"""
    gen = torch.Generator().manual_seed(3)
    pool = torch.tensor([0, 1, 1, 2, 2, 3, 4, 5, 6])
    for G, L, n in ((1, 9, 2), (3, 7, 5), (2, 1, 4)):
        commands = pool[torch.randint(0, len(pool), (2 * G, L), generator=gen)].float()
        args = torch.rand(2 * G, L, 11, generator=gen, dtype=torch.float64).requires_grad_(True)
        points, counts = GR.sample_points64(commands, args, n, groups=G)
        dpoints = torch.randn(points.shape, generator=gen, dtype=torch.float64)       # (rows past counts: never read)
        want, = torch.autograd.grad((points * dpoints).sum(), args)
        got = GR.sample_points_bwd(commands, dpoints, n, groups=G, as_double=True)
        assert int(counts.sum()) > 0 and (got - want).abs().max().item() < 1e-12


def test_gradient_reaches_args_and_counts_carry_none(metric_grad_ops):
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    ax, ay = args[i].clone().requires_grad_(True), args[j].clone().requires_grad_(True)
    px, nx = metrics.sample_points(commands[i], ax, N)
    py, ny = metrics.sample_points(commands[j], ay, N)
    assert px.requires_grad and px.grad_fn is not None and nx.grad_fn is None and not nx.requires_grad
    out = metrics.chamfer(px, nx, py, ny)
    assert out.requires_grad
    out.sum().backward()
    err = max((ax.grad.double() - torch.from_numpy(g["grad_x"])).abs().max().item(),
              (ay.grad.double() - torch.from_numpy(g["grad_y"])).abs().max().item())
    assert err <= grad_bound(g), err
    assert torch.equal(ax.grad[:, :, :5], torch.zeros_like(ax.grad[:, :, :5]))
    # one side only
    ax2 = args[i].clone().requires_grad_(True)
    px2, _ = metrics.sample_points(commands[i], ax2, N)
    metrics.chamfer(px2, nx, py.detach(), ny).sum().backward()
    assert torch.equal(ax2.grad, ax.grad)


def test_forward_only_calls_return_what_they_returned(metric_grad_ops, monkeypatch):
    """int64 inputs, no_grad and inputs that do not require grad stay on ops.sample_points / ops.chamfer"""
    import deepsvg_amd.ops as ops
    g, commands, args, _ = golden_grad()
    for name in GR.NAMES:
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("a forward-only call reached a backward op"))
    want_p, want_c = MR.sample_points(commands, args, N)
    want = MR.chamfer(want_p, want_c, want_p.flip(0).contiguous(), want_c.flip(0).contiguous())
    a = args.clone().requires_grad_(True)
    with torch.no_grad():
        p, c = metrics.sample_points(commands, a, N)
        out = metrics.chamfer(p, c, p.flip(0), c.flip(0))
    assert torch.equal(p, want_p) and torch.equal(c, want_c) and not p.requires_grad
    assert torch.equal(out, want, ) and not out.requires_grad
    p, c = metrics.sample_points(commands, args, N)
    assert torch.equal(p, want_p) and p.grad_fn is None
    assert torch.equal(metrics.chamfer(p, c, p.flip(0), c.flip(0)), want)
    ci, ai = commands.long(), args.round().long()
    pi, cnt = metrics.sample_points(ci, ai, N)
    wi, _ = MR.sample_points(ci, ai, N)
    assert torch.equal(pi, wi) and torch.equal(cnt, want_c) and pi.grad_fn is None


def _with_an_empty_icon():
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    commands_x, args_x = commands[i].clone(), args[i].clone()
    commands_x[1] = torch.where((commands_x[1] == 1) | (commands_x[1] == 2), torch.zeros(()), commands_x[1])    # only m: no points
    ty, tn = MR.sample_points(commands[j], args[j], N)
    return commands_x, args_x, ty, tn


def test_empty_cloud_gives_zero_rows_and_a_finite_loss(metric_grad_ops):
    commands_x, args_x, ty, tn = _with_an_empty_icon()
    a = args_x.clone().requires_grad_(True)
    res = metrics.chamfer_loss(commands_x, a, ty, tn, N)
    assert res["loss"].dim() == 0 and res["per_icon"].shape == (6,) and res["valid"].dtype == torch.bool
    assert res["valid"].tolist() == [True, False, True, True, True, True] and torch.isnan(res["per_icon"][1]).item()
    assert torch.isfinite(res["loss"]).item()
    assert abs(res["loss"].item() - res["per_icon"][res["valid"]].double().mean().item()) < 1e-4
    res["loss"].backward()
    assert bool(torch.isfinite(a.grad).all()) and torch.equal(a.grad[1], torch.zeros_like(a.grad[1]))
    assert float(a.grad[0].abs().max()) > 0
    # the op itself: zero rows on the empty icon even when dout is NaN there
    import deepsvg_amd.ops as ops
    px, nx = MR.sample_points(commands_x, args_x, N)
    _, idx_x, idx_y = ops.chamfer_nn(px, nx, ty, tn)
    dout = torch.ones(6)
    dout[1] = float("nan")
    dpx, dpy = ops.chamfer_bwd(px, nx, ty, tn, idx_x, idx_y, dout)
    assert torch.equal(dpx[1], torch.zeros_like(dpx[1])) and torch.equal(dpy[1], torch.zeros_like(dpy[1]))
    assert bool(torch.isfinite(dpx).all() & torch.isfinite(dpy).all())


def test_refine_lowers_the_loss_and_leaves_the_rest_alone(metric_grad_ops):
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    ty, tn = MR.sample_points(commands[j], args[j], N)
    before = args[i].clone()
    refined, history = metrics.refine(commands[i], args[i], ty, tn, steps=20, lr=0.1, n=N)
    assert torch.equal(args[i], before), "refine changed its input"
    assert refined.shape == before.shape and refined.dtype == torch.float32 and not refined.requires_grad
    assert history.shape == (20,) and bool(torch.isfinite(history).all())
    print(f"refine, 20 steps: loss {history[0].item():.4f} -> {history[-1].item():.4f}")
    assert history[-1].item() < history[0].item()
    assert torch.equal(refined[:, :, :5], before[:, :, :5]), "columns 0-4 moved"
    rows = torch.arange(commands.shape[1]).unsqueeze(0) >= torch.from_numpy(golden()[0]["lens"])[i].long().unsqueeze(1)
    assert torch.equal(refined[rows], before[rows]), "padding rows moved"
    assert not torch.equal(refined, before)
