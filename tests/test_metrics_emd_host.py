"""The ordered point loss and the length losses of deepsvg_amd.metrics on CPU: the float64 restatements (tests/emd_ref.py)
against the reference's own results (tests/golden/metrics/metrics_emd.npz, make_golden_metrics_emd.py), and the autograd
wiring of emd / emd_loss / polyline_length / svg_length_loss / continuity_loss / refine(loss="emd") with the ops replaced
by restatements.

Bounds: the loss within CHAMFER_ATOL (1e-4, as for the Chamfer distance: distances of at most 362 from fp32 points); the
gradient within 4 x `ref_spread`, the fixture's own measure of what the reference's fp32 sampling costs it; matched
indices and the shift exactly - the fixture's margins (asserted below) put every choice far from a tie."""
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import metrics
from tests import emd_ref as ER
from tests import helpers as H
from tests import metrics_grad_ref as GR
from tests import metrics_ref as MR
from tests.test_metrics_host import CHAMFER_ATOL

GOLDEN_EMD = os.path.join(H.GOLDEN_DIR, "metrics", "metrics_emd.npz")
N = 4
PUBLIC = ("emd", "emd_loss", "polyline_length", "svg_length_loss", "continuity_loss")
SYMBOLS = ("dsvg_emd_workspace_bytes", "dsvg_emd", "dsvg_emd_bwd", "dsvg_polyline_length", "dsvg_polyline_length_bwd")
API = tuple(getattr(metrics, name) for name in PUBLIC)          # without the feature nothing below can run


@pytest.fixture
def emd_ops(emulated_ops):
    saved = ER.install()
    yield
    ER.restore(saved)


def golden_emd():
    """-> fixture dict of numpy arrays, and commands_x, args_x, commands_y, args_y as tensors"""
    g = dict(np.load(GOLDEN_EMD, allow_pickle=False))
    return (g,) + tuple(torch.from_numpy(g[k]) for k in ("commands_x", "args_x", "commands_y", "args_y"))


def grad_bound(g):
    return 4.0 * float(g["ref_spread"])


def fixture_clouds():
    g, cx, ax, cy, ay = golden_emd()
    px, nx = MR.sample_points(cx, ax, N)                   # fp32 points, as the kernel's
    py, ny = MR.sample_points(cy, ay, N)
    return g, cx, px, nx, py, ny


def test_public_surface():
    from deepsvg_amd import lib, ops
    assert all(name in metrics.__all__ for name in PUBLIC) and all(callable(f) for f in API)
    assert lib.ABI_VERSION >= 15 and all(name in lib.SIGNATURES for name in SYMBOLS)
    assert all(callable(getattr(ops, name)) for name in ER.NAMES)


def test_fixture_margins():
    g = golden_emd()[0]
    assert float(g["shift_gap"]) >= 1e-3 and float(g["match_gap"]) >= 1e-4
    assert float(g["min_area"]) >= 1.0 and float(g["min_dist"]) >= 1e-2
    assert 0 < float(g["ref_spread"]) < 1e-5 and 0 <= float(g["loss_spread"]) < CHAMFER_ATOL
    assert g["flip"].any() and not g["flip"].all(), "both orientations of the target must occur"
    assert len(g["pairs"]) == 5 and not np.isnan(g["grad"]).any() and not np.isnan(g["grad_w"]).any()
    assert os.path.getsize(GOLDEN_EMD) < 32 * 1024


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_matches_the_reference(weighted):
    g, cx, px, nx, py, ny = fixture_clouds()
    sfx = "_w" if weighted else ""
    out, shift, matched, t = ER.emd(px, nx, py, ny, weighted, as_double=True)
    err = (out - torch.from_numpy(g["loss" + sfx])).abs().max().item()
    print(f"restated loss vs the reference: max abs err {err:.3e} (bound {CHAMFER_ATOL:.1e})")
    assert err <= CHAMFER_ATOL
    assert torch.equal(matched, torch.from_numpy(g["matched"])) and torch.equal(shift, torch.from_numpy(g["shift"]))
    dpx = ER.emd_bwd(px, nx, ny, t, shift, torch.ones(len(nx)), weighted, as_double=True)
    grad = GR.sample_points_bwd(cx, dpx.float(), N, as_double=True)
    gerr = (grad - torch.from_numpy(g["grad" + sfx])).abs().max().item()
    print(f"restated gradient vs autograd on the reference's indices: max abs err {gerr:.3e} (bound {grad_bound(g):.3e})")
    assert gerr <= grad_bound(g)
    # the kernel's arithmetic (fp32 terms, float64 sums) makes the same choices on these margins
    out_f, shift_f, matched_f, _ = ER.emd(px, nx, py, ny, weighted, float_terms=True, as_double=True)
    assert torch.equal(shift_f, shift) and torch.equal(matched_f, matched)
    assert (out_f - out).abs().max().item() <= 8 * 2.0 ** -24 * out.max().item()


def test_restated_lengths_match_the_reference():
    g, cx, px, nx, py, ny = fixture_clouds()
    lx, ly = ER.polyline_length(px, nx, as_double=True), ER.polyline_length(py, ny, as_double=True)
    err = ((ly - lx).abs() / ly - torch.from_numpy(g["length_loss"])).abs().max().item()
    cerr = (lx / (nx - 1) - torch.from_numpy(g["continuity"])).abs().max().item()
    print(f"svg_length_loss err {err:.3e}, continuity_loss err {cerr:.3e}")
    assert err <= 1e-5 and cerr <= CHAMFER_ATOL       # a ratio of lengths of ~1e3 units with fp32 sums; a mean distance


class _Emd64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, px, nx, py, ny, weighted):
        out, shift, _, t = ER.emd(px, nx, py, ny, weighted, as_double=True)
        ctx.save_for_backward(px, nx, ny, t, shift)
        ctx.weighted = weighted
        return out

    @staticmethod
    def backward(ctx, dout):
        return ER.emd_bwd(*ctx.saved_tensors, dout, ctx.weighted, as_double=True), None, None, None, None


class _Length64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, n):
        ctx.save_for_backward(p, n)
        return ER.polyline_length(p, n, as_double=True)

    @staticmethod
    def backward(ctx, dout):
        return ER.polyline_length_bwd(*ctx.saved_tensors, dout, as_double=True), None


@pytest.mark.parametrize("weighted", [False, True])
def test_gradcheck_of_the_restated_emd(weighted):
    """on the fixture's clouds: its margins keep every choice fixed under gradcheck's 1e-6 perturbations"""
    g, cx, px, nx, py, ny = fixture_clouds()
    x = px.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: _Emd64.apply(v, nx, py.double(), ny, weighted), (x,), eps=1e-6, atol=1e-6)


def test_gradcheck_of_the_restated_polyline_length():
    g, cx, px, nx, py, ny = fixture_clouds()
    x = px.double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: _Length64.apply(v, nx), (x,), eps=1e-6, atol=1e-6)


def test_gradient_reaches_args_through_emd(emd_ops):
    g, cx, ax, cy, ay = golden_emd()
    ty, tn = MR.sample_points(cy, ay, N)
    for weighted, sfx in ((False, ""), (True, "_w")):
        a = ax.clone().requires_grad_(True)
        px, nx = metrics.sample_points(cx, a, N)
        loss, matched, shift = metrics.emd(px, nx, ty, tn, first_point_weight=weighted, return_matched_indices=True)
        assert loss.requires_grad and not matched.requires_grad and not shift.requires_grad
        assert matched.dtype == torch.int32 and shift.dtype == torch.int32 and loss.dtype == torch.float32
        assert torch.equal(matched, torch.from_numpy(g["matched"])) and torch.equal(shift, torch.from_numpy(g["shift"]))
        loss.sum().backward()
        err = (a.grad.double() - torch.from_numpy(g["grad" + sfx])).abs().max().item()
        assert err <= grad_bound(g), err
        assert torch.equal(a.grad[:, :, :5], torch.zeros_like(a.grad[:, :, :5]))
        # the same bits without gradients, through the same op
        with torch.no_grad():
            again = metrics.emd(px, nx, ty, tn, first_point_weight=weighted)
        assert torch.equal(again, loss.detach()) and not again.requires_grad
        assert torch.equal(metrics.emd(px.detach(), nx, ty, tn, first_point_weight=weighted), loss.detach())
    # a target that requires grad gets none: it is a constant
    ty2 = ty.clone().requires_grad_(True)
    a = ax.clone().requires_grad_(True)
    px, nx = metrics.sample_points(cx, a, N)
    metrics.emd(px, nx, ty2, tn).sum().backward()
    assert ty2.grad is None and a.grad is not None


def test_emd_loss_masks_empty_clouds(emd_ops):
    g, cx, ax, cy, ay = golden_emd()
    ty, tn = MR.sample_points(cy, ay, N)
    cx = cx.clone()
    cx[1] = torch.where((cx[1] == 1) | (cx[1] == 2), torch.zeros(()), cx[1])          # only m: an empty pred cloud
    tn = tn.clone()
    tn[3] = 0                                                                         # an empty target
    a = ax.clone().requires_grad_(True)
    res = metrics.emd_loss(cx, a, ty, tn, N)
    assert res["loss"].dim() == 0 and res["per_icon"].shape == (5,) and res["valid"].tolist() == [True, False, True, False, True]
    assert res["per_icon"][1].item() == 0.0 and torch.isnan(res["per_icon"][3]).item()          # loss.py:25-26; chamfer's NaN
    want = torch.from_numpy(g["loss"])[[0, 2, 4]].mean().item()
    assert abs(res["loss"].item() - want) <= CHAMFER_ATOL
    res["loss"].backward()
    assert bool(torch.isfinite(a.grad).all())
    assert torch.equal(a.grad[1], torch.zeros_like(a.grad[1])) and torch.equal(a.grad[3], torch.zeros_like(a.grad[3]))
    assert float(a.grad[0].abs().max()) > 0
    # no valid icon at all: NaN, as chamfer_loss
    none = metrics.emd_loss(cx, ax, ty, torch.zeros_like(tn), N)
    assert torch.isnan(none["loss"]).item() and not bool(none["valid"].any())


def test_restated_empty_cloud_conventions():
    px, py = torch.rand(3, 5, 2), torch.rand(3, 7, 2)
    nx, ny = torch.tensor([0, 4, 0], dtype=torch.int32), torch.tensor([7, 0, 0], dtype=torch.int32)
    out, shift, matched, t = ER.emd(px, nx, py, ny)
    assert out[0].item() == 0.0 and torch.isnan(out[1]).item() and out[2].item() == 0.0
    assert shift.tolist() == [0, 0, 0] and bool((matched == -1).all())
    dout = torch.tensor([1.0, float("nan"), 1.0])
    assert torch.equal(ER.emd_bwd(px, nx, ny, t, shift, dout), torch.zeros(3, 5, 2))
    # a single target point, and a target of equal points: every pred point matches index 0 of the reversed target
    ny1 = torch.tensor([1, 3, 1], dtype=torch.int32)
    py[1, :3] = py[1, 0]
    nx1 = torch.tensor([2, 4, 1], dtype=torch.int32)
    _, _, matched, _ = ER.emd(px, nx1, py, ny1)
    assert matched[0, :2].tolist() == [0, 0] and matched[1, :4].tolist() == [2, 2, 2, 2] and matched[2, 0].item() == 0


def test_length_losses(emd_ops):
    g, cx, ax, cy, ay = golden_emd()
    ty, tn = MR.sample_points(cy, ay, N)
    a = ax.clone().requires_grad_(True)
    px, nx = metrics.sample_points(cx, a, N)
    length = metrics.polyline_length(px, nx)
    assert length.requires_grad and length.dtype == torch.float32 and length.shape == (5,)
    ll = metrics.svg_length_loss(px, nx, ty, tn)
    cl = metrics.continuity_loss(px, nx)
    assert (ll.double() - torch.from_numpy(g["length_loss"])).abs().max().item() <= 1e-5
    assert (cl.double() - torch.from_numpy(g["continuity"])).abs().max().item() <= CHAMFER_ATOL
    (ll.sum() + cl.sum()).backward()
    assert bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().max()) > 0
    # autograd through the plain-torch statement of the two losses on the same points
    b = ax.clone().requires_grad_(True)
    qx, _ = metrics.sample_points(cx, b, N)
    total = 0
    for i in range(5):
        p, q = qx[i, :nx[i]].double(), ty[i, :tn[i]].double()
        lp, lq = (p[1:] - p[:-1]).norm(dim=-1).sum(), (q[1:] - q[:-1]).norm(dim=-1).sum()
        total = total + (lq - lp).abs() / lq + (p[1:] - p[:-1]).norm(dim=-1).mean()
    total.backward()
    assert (a.grad - b.grad).abs().max().item() <= 1e-5
    # 0 and 1 point: length 0, continuity NaN; a zero-length target: svg_length_loss NaN, zero gradient
    p = px.detach().clone().requires_grad_(True)
    few = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32)
    assert metrics.polyline_length(p, few)[:2].tolist() == [0.0, 0.0]
    c = metrics.continuity_loss(p, few)
    assert torch.isnan(c[:2]).all().item() and bool(torch.isfinite(c[2:]).all())
    z = metrics.svg_length_loss(p, nx, ty, torch.ones_like(tn))
    assert bool(torch.isnan(z).all())
    z.sum().backward()
    assert torch.equal(p.grad, torch.zeros_like(p.grad))
    with torch.no_grad():
        assert torch.equal(metrics.polyline_length(px, nx), length.detach())


def test_refine_with_the_ordered_loss(emd_ops):
    g, cx, ax, cy, ay = golden_emd()
    ty, tn = MR.sample_points(cy, ay, N)
    before = ax.clone()
    refined, history = metrics.refine(cx, ax, ty, tn, steps=20, lr=0.1, n=N, loss="emd")
    assert torch.equal(ax, before), "refine changed its input"
    assert history.shape == (20,) and bool(torch.isfinite(history).all())
    assert abs(history[0].item() - float(g["loss"].mean())) <= CHAMFER_ATOL
    print(f"refine(loss='emd'), 20 steps: loss {history[0].item():.4f} -> {history[-1].item():.4f}")
    assert history[-1].item() < history[0].item()
    assert torch.equal(refined[:, :, :5], before[:, :, :5]) and not torch.equal(refined, before)


def test_refine_rejects_an_unknown_loss(emd_ops):
    g, cx, ax, cy, ay = golden_emd()
    ty, tn = MR.sample_points(cy, ay, N)
    with pytest.raises(ValueError):
        metrics.refine(cx, ax, ty, tn, steps=1, n=N, loss="bogus")


def test_refine_default_is_the_chamfer_loop(emd_ops):
    g, cx, ax, cy, ay = golden_emd()
    ty, tn = MR.sample_points(cy, ay, N)
    refined, history = metrics.refine(cx, ax, ty, tn, steps=5, lr=0.1, n=N)
    want = ax.detach().float().clone().requires_grad_(True)
    opt = torch.optim.Adam([want], lr=0.1)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = metrics.chamfer_loss(cx, want, ty, tn, N)["loss"]
        loss.backward()
        losses.append(loss.detach())
        opt.step()
    assert torch.equal(refined, want.detach()) and torch.equal(history, torch.stack(losses))
    explicit, h2 = metrics.refine(cx, ax, ty, tn, steps=5, lr=0.1, n=N, loss="chamfer")
    assert torch.equal(explicit, refined) and torch.equal(h2, history)
