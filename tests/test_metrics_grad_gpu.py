"""The gradient of deepsvg_amd.metrics on a real MI355X: dsvg_chamfer_nn, dsvg_chamfer_bwd and dsvg_sample_points_bwd
(csrc/metrics.hip) against the reference's own autograd (tests/golden/metrics/metrics_grad.npz) and the float64
restatements of tests/metrics_grad_ref.py, their conventions and exactness properties, and chamfer_loss / refine end to
end.  Every test prints the largest error it saw before it asserts.

Bounds:
  end to end          4 x ref_spread of the fixture (what the reference's own fp32 sampling costs its gradient; the kernel
                      rounds in another order in two places: Horner sampling, unit vector from fp32 differences)
  chamfer_nn          `out` equal to ops.chamfer's in bits; an index is valid when its distance is within 1e-4 (the
                      forward's Chamfer tolerance) of the float64 minimum
  chamfer_bwd         against the restatement FED THE KERNEL'S OWN INDICES: every term is a unit vector over a count, off by
                      a few fp32 ulps of 1 / count, and at most n_x + n_y terms add:
                      8 * 2^-24 * (1 + (n_x + n_y) / min(n_x, n_y)) per element at dout = 1
  sample_points_bwd   n * 2^-22 * max|dP|: n products of weights <= 1 per element
"""
import numpy as np
import pytest
import torch

from deepsvg_amd import lib, metrics, ops
from tests import metrics_grad_ref as GR
from tests import metrics_ref as MR
from tests.test_metrics_gpu import _random_sequences
from tests.test_metrics_grad_host import N, golden_grad, grad_bound
from tests.test_metrics_host import CHAMFER_ATOL
from tests.test_metrics_host import GOLDEN as GOLDEN_POINTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


# ---- end to end against the reference ---------------------------------------------------------------------------------------
def test_gradient_matches_the_reference_autograd(gpu_device):
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    cx, cy = commands[i].to(DEV), commands[j].to(DEV)
    ax, ay = args[i].to(DEV).requires_grad_(True), args[j].to(DEV).requires_grad_(True)
    px, nx = metrics.sample_points(cx, ax, N)
    py, ny = metrics.sample_points(cy, ay, N)
    assert px.requires_grad and nx.grad_fn is None
    out = metrics.chamfer(px, nx, py, ny)
    out.sum().backward()
    ex = (ax.grad.cpu().double() - torch.from_numpy(g["grad_x"])).abs().max().item()
    ey = (ay.grad.cpu().double() - torch.from_numpy(g["grad_y"])).abs().max().item()
    el = (out.detach().cpu().double() - torch.from_numpy(g["loss"])).abs().max().item()
    print(f"d chamfer / d args vs the reference's autograd: max abs err {ex:.3e} / {ey:.3e} (bound {grad_bound(g):.3e}, "
          f"ref_spread {float(g['ref_spread']):.3e}); loss err {el:.3e}")
    assert max(ex, ey) <= grad_bound(g)
    assert el <= CHAMFER_ATOL
    with torch.no_grad():                               # the differentiable call has the forward-only call's bits
        p0, n0 = metrics.sample_points(cx, ax, N)
        live = torch.arange(p0.shape[1], device=DEV).unsqueeze(0) < n0.unsqueeze(1)      # rows past counts hold anything
        assert torch.equal(p0[live], px.detach()[live]) and torch.equal(n0, nx)
        assert torch.equal(metrics.chamfer(p0, n0, py.detach(), ny).view(torch.int32), out.detach().view(torch.int32))


# ---- chamfer_nn / chamfer_bwd ---------------------------------------------------------------------------------------------
# the 64-lane chunk, the 1,024-point slice and tile, their off-by-ones, 3 slices, and an empty cloud per batch
BATCHES = [[(1, 2049), (63, 64), (0, 65)],
           [(1023, 1025), (1024, 1024), (65, 1)],
           [(2049, 1023), (1025, 63), (64, 0)]]


@pytest.fixture(scope="module")
def cloud_batches():
    """per batch: px, nx, py, ny (caps unequal and larger than every count, NaN past the counts) and the float64 nearest
    distances of both directions, brute force, computed once"""
    gen = torch.Generator().manual_seed(11)
    out = []
    for sizes in BATCHES:
        capx, capy = max(s[0] for s in sizes) + 5, max(s[1] for s in sizes) + 2
        px, py = torch.rand(3, capx, 2, generator=gen) * 255, torch.rand(3, capy, 2, generator=gen) * 255
        nx = torch.tensor([s[0] for s in sizes], dtype=torch.int32)
        ny = torch.tensor([s[1] for s in sizes], dtype=torch.int32)
        near = []
        for b, (cx, cy) in enumerate(sizes):
            px[b, cx:], py[b, cy:] = float("nan"), float("nan")        # rows past the counts must never be read
            if cx == 0 or cy == 0:
                near.append(None)
                continue
            d = torch.cdist(px[b, :cx].double(), py[b, :cy].double())
            near.append((d.min(1).values, d.min(0).values))
        out.append((px, nx, py, ny, near))
    return out


def _dist(a, b):
    return (a.double() - b.double()).norm(dim=-1)


def test_chamfer_nn_has_chamfers_bits_and_valid_indices(gpu_device, cloud_batches):
    worst = 0.0
    for (px, nx, py, ny, near), sizes in zip(cloud_batches, BATCHES):
        dpx, dnx, dpy, dny = _dev(px, nx, py, ny)
        out, idx_x, idx_y = ops.chamfer_nn(dpx, dnx, dpy, dny)
        want = ops.chamfer(dpx, dnx, dpy, dny)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "chamfer_nn's out differs from chamfer's in bits"
        assert idx_x.dtype == torch.int32 and idx_x.shape == px.shape[:2] and idx_y.shape == py.shape[:2]
        idx_x, idx_y = idx_x.cpu().long(), idx_y.cpu().long()
        for b, (cx, cy) in enumerate(sizes):
            if cx == 0 or cy == 0:
                assert torch.isnan(out[b]).item()
                continue
            jx, iy = idx_x[b, :cx], idx_y[b, :cy]
            assert bool(((jx >= 0) & (jx < cy)).all()) and bool(((iy >= 0) & (iy < cx)).all()), "index outside its cloud"
            ex = (_dist(px[b, :cx], py[b, jx]) - near[b][0]).max().item()
            ey = (_dist(py[b, :cy], px[b, iy]) - near[b][1]).max().item()
            worst = max(worst, ex, ey)
    print(f"chamfer_nn: distance to the chosen point - float64 minimum, largest {worst:.3e}")
    assert worst <= 1e-4


def test_chamfer_bwd_matches_the_restatement_on_its_own_indices(gpu_device, cloud_batches):
    worst_ratio = 0.0
    for (px, nx, py, ny, near), sizes in zip(cloud_batches, BATCHES):
        for b, (cx, cy) in enumerate(sizes):            # (the derivation of the bound assumes a unit vector is well defined)
            if cx and cy:
                assert min(near[b][0].min().item(), near[b][1].min().item()) >= 1e-2, "inputs: a nearest distance below 1e-2"
        dev = _dev(px, nx, py, ny)
        _, idx_x, idx_y = ops.chamfer_nn(*dev)
        dout = torch.ones(3)
        dpx, dpy = ops.chamfer_bwd(*dev, idx_x, idx_y, dout.to(DEV))
        want_x, want_y = GR.chamfer_bwd(px, nx, py, ny, idx_x.cpu(), idx_y.cpu(), dout, as_double=True)
        for b, (cx, cy) in enumerate(sizes):
            bound = 8 * EPS * (1 + (cx + cy) / min(cx, cy)) if cx and cy else 0.0
            err = max((dpx[b].cpu().double() - want_x[b]).abs().max().item(), (dpy[b].cpu().double() - want_y[b]).abs().max().item())
            print(f"chamfer_bwd {cx} x {cy}: max abs err {err:.3e} (bound {bound:.3e})")
            assert err <= bound
            worst_ratio = max(worst_ratio, err / bound if bound else 0.0)
        for grad, cnt in ((dpx.cpu(), nx), (dpy.cpu(), ny)):
            past = torch.arange(grad.shape[1]).unsqueeze(0) >= cnt.unsqueeze(1)
            assert torch.equal(grad[past], torch.zeros(int(past.sum()), 2)), "rows past the counts are not zero"
    print(f"chamfer_bwd: largest err / bound {worst_ratio:.3f}")


def test_chamfer_bwd_conventions_on_lattice_points(gpu_device):
    nan = float("nan")
    # icon 0: x_0 is equidistant from y_0 and y_1 -> its direct term points away from y_0
    # icon 1: y_0 is equidistant from x_0 and x_1 -> x_0 receives y_0's term, x_1 its direct term only
    # icon 2: an empty cloud, dout = NaN
    px = torch.tensor([[[5., 5.], [nan, nan], [nan, nan]], [[6., 5.], [4., 5.], [nan, nan]], [[1., 1.], [2., 2.], [nan, nan]]])
    py = torch.tensor([[[6., 5.], [4., 5.], [5., 9.], [nan, nan]], [[5., 5.], [nan, nan], [nan, nan], [nan, nan]],
                       [[nan, nan]] * 4])
    nx, ny = torch.tensor([1, 2, 2], dtype=torch.int32), torch.tensor([3, 1, 0], dtype=torch.int32)
    dev = _dev(px, nx, py, ny)
    out, idx_x, idx_y = ops.chamfer_nn(*dev)
    assert idx_x[0, 0].item() == 0 and idx_y[1, 0].item() == 0, "a tie did not go to the lowest index"
    assert idx_y[0, :3].tolist() == [0, 0, 0] and idx_x[1, :2].tolist() == [0, 0]
    dout = torch.tensor([1.0, 1.0, nan])
    dpx, dpy = (t.cpu() for t in ops.chamfer_bwd(*dev, idx_x, idx_y, dout.to(DEV)))
    # icon 0: (-1, 0) + ((-1, 0) + (1, 0) + (0, -1)) / 3, added in ascending j
    third = torch.tensor(1.0) / torch.tensor(3.0)
    want0 = torch.stack([(torch.tensor(-1.0) + -third) + third + 0.0, (torch.tensor(0.0) + 0.0) + 0.0 - third])
    assert torch.equal(dpx[0, 0], want0), (dpx[0, 0], want0)
    # y_0 = its own (1, 0) / 3 and, as x_0's nearest point, - u(x_0, y_0) / 1; y_1 and y_2 their own terms only
    assert torch.equal(dpy[0, :3], torch.tensor([[1., 0.], [-1., 0.], [0., 1.]]) / 3 + torch.tensor([[1., 0.], [0., 0.], [0., 0.]]))
    assert torch.equal(dpx[1, :2], torch.tensor([[1.5, 0.], [-0.5, 0.]])), dpx[1]      # (1, 0) / 2 + (1, 0); (-1, 0) / 2
    assert torch.equal(dpy[1, 0], torch.tensor([-1., 0.]))          # (-1, 0) + (-1, 0) / 2 + (1, 0) / 2
    assert torch.equal(dpx[2], torch.zeros(3, 2)) and torch.equal(dpy[2], torch.zeros(4, 2)), "empty cloud, dout = NaN"
    assert torch.equal(dpx[0, 1:], torch.zeros(2, 2)) and torch.equal(dpy[1, 1:], torch.zeros(3, 2)), "rows past the counts"
    # a cloud against itself: every nearest distance is zero, every term is zero
    gen = torch.Generator().manual_seed(2)
    x = torch.randint(0, 256, (2, 1030, 2), generator=gen).float().to(DEV)
    n = torch.tensor([1025, 300], dtype=torch.int32, device=DEV)
    y = x.clone()
    out, idx_x, idx_y = ops.chamfer_nn(x, n, y, n)
    gx, gy = ops.chamfer_bwd(x, n, y, n, idx_x, idx_y, torch.full((2,), 3.0, device=DEV))
    assert torch.equal(out.cpu(), torch.zeros(2))
    assert torch.equal(gx.cpu(), torch.zeros(2, 1030, 2)) and torch.equal(gy.cpu(), torch.zeros(2, 1030, 2))


def test_chamfer_bwd_is_exact_where_it_can_be(gpu_device, cloud_batches):
    px, nx, py, ny, _ = cloud_batches[2]
    dev = _dev(px, nx, py, ny)
    dout = torch.tensor([0.5, -1.25, 3.0], device=DEV)
    _, idx_x, idx_y = ops.chamfer_nn(*dev)
    gx, gy = ops.chamfer_bwd(*dev, idx_x, idx_y, dout)
    _, idx_x2, idx_y2 = ops.chamfer_nn(*dev)
    gx2, gy2 = ops.chamfer_bwd(*dev, idx_x2, idx_y2, dout)
    bits = lambda t: t.view(torch.int32)                                                   # noqa: E731
    live_x = (torch.arange(px.shape[1]).unsqueeze(0) < nx.unsqueeze(1)).to(DEV) & (ny > 0).unsqueeze(1).to(DEV)
    assert torch.equal(idx_x[live_x], idx_x2[live_x])
    assert torch.equal(bits(gx), bits(gx2)) and torch.equal(bits(gy), bits(gy2)), "two runs differ in bits"
    swapped = (dev[2], dev[3], dev[0], dev[1])
    _, sidx_x, sidx_y = ops.chamfer_nn(*swapped)
    sgx, sgy = ops.chamfer_bwd(*swapped, sidx_x, sidx_y, dout)
    assert torch.equal(bits(gx), bits(sgy)) and torch.equal(bits(gy), bits(sgx)), "d chamfer(x, y) / dx != second gradient of chamfer(y, x)"


def test_training_call_builds_no_distance_matrix(gpu_device):
    gen = torch.Generator().manual_seed(6)
    px, py = (torch.rand(4, 2431, 2, generator=gen) * 255).to(DEV), (torch.rand(4, 2431, 2, generator=gen) * 255).to(DEV)
    nx = torch.tensor([2400, 2431, 2399, 2405], dtype=torch.int32, device=DEV)
    ny = torch.tensor([2431, 2390, 2400, 2411], dtype=torch.int32, device=DEV)
    dout = torch.ones(4, device=DEV)
    ops.chamfer_bwd(px, nx, py, ny, *ops.chamfer_nn(px, nx, py, ny)[1:], dout)          # (code objects loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, idx_x, idx_y = ops.chamfer_nn(px, nx, py, ny)
    gx, gy = ops.chamfer_bwd(px, nx, py, ny, idx_x, idx_y, dout)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    need = idx_x.numel() * 4 * 2 + gx.numel() * 4 * 2
    print(f"chamfer_nn + chamfer_bwd of 4 x ~2,400 points: peak allocation grew by {grown} bytes (indices + gradients {need})")
    assert grown < need + (64 << 10) and bool(torch.isfinite(gx).all())                 # one icon's matrix alone: 23 MB


# ---- sample_points_bwd ----------------------------------------------------------------------------------------------------
def _sample_points_bwd_nan_filled(commands, dpoints, n, G):
    """the C entry on an output filled with NaN beforehand: every element must be written"""
    dargs = torch.full((commands.shape[0], commands.shape[1], 11), float("nan"), device=DEV)
    lib.check(lib.load().dsvg_sample_points_bwd(commands.data_ptr(), commands.shape[0] // G, G, commands.shape[1], n,
                                                dpoints.data_ptr(), dargs.data_ptr(), None), "dsvg_sample_points_bwd")
    torch.cuda.synchronize()
    return dargs


def _check_bwd_against_restatement(commands, n, seed):
    """-> err / bound; dpoints is NaN past the counts: those rows must not be read"""
    B, G, L = commands.shape
    c = commands.reshape(B * G, L).float()
    _, counts = MR.sample_points(c, torch.zeros(B * G, L, 11), n=n, groups=G)
    cap = G * (L * (n - 1) + 1)
    dpoints = torch.randn(B, cap, 2, generator=torch.Generator().manual_seed(seed))
    dpoints[torch.arange(cap).unsqueeze(0) >= counts.unsqueeze(1)] = float("nan")
    want = GR.sample_points_bwd(c, dpoints, n=n, groups=G, as_double=True)
    got = _sample_points_bwd_nan_filled(c.to(DEV), dpoints.to(DEV), n, G).cpu()
    assert not bool(torch.isnan(got).any()), "an element was not written (or a row past the counts was read)"
    assert torch.equal(got[:, :, :5], torch.zeros(B * G, L, 5)), "columns 0-4"
    assert torch.equal(got[want == 0], torch.zeros(int((want == 0).sum()))), "an untouched element is not an exact zero"
    live = ~torch.isnan(dpoints)
    bound = n * 2.0 ** -22 * (dpoints[live].abs().max().item() if bool(live.any()) else 0.0)
    err = (got.double() - want).abs().max().item()
    assert err <= bound, (err, bound)
    return err / bound if bound else 0.0


@pytest.mark.parametrize("n", [2, 7, 10, 64])
def test_sample_points_bwd_matches_the_restatement(gpu_device, n):
    worst = 0.0
    for B in (1, 5):
        for G in (1, 8):
            for L in (1, 32, 66):
                commands, _ = _random_sequences(B, G, L, seed=1000 * B + 100 * G + L + n)
                worst = max(worst, _check_bwd_against_restatement(commands, n, seed=B + G + L))
    print(f"sample_points_bwd vs float64 restatement n={n}: largest err / bound {worst:.3e}")


def test_sample_points_bwd_at_2048_tokens_per_cloud(gpu_device):
    commands, _ = _random_sequences(2, 8, 256, seed=77)
    print(f"sample_points_bwd G=8 L=256: err / bound {_check_bwd_against_restatement(commands, 10, seed=1):.3e}")


def test_sample_points_bwd_start_point_rule(gpu_device):
    n = 4
    # row 0: l at row 0 (its start is the constant (0, 0)), then c; row 1: SOS, m, l, c, z, EOS; row 2: nothing drawn
    commands = torch.tensor([[1, 2, 4, 4, 4, 4], [5, 0, 1, 2, 6, 4], [5, 0, 6, 4, 4, 4]], dtype=torch.float32)
    dpoints = torch.zeros(3, 6 * (n - 1) + 1, 2)
    dpoints[:2, :2 * (n - 1) + 1] = torch.arange(1, 2 * (2 * (n - 1) + 1) + 1, dtype=torch.float32).view(1, -1, 2)
    dpoints[2] = float("nan")                           # count 0: nothing is read
    got = _sample_points_bwd_nan_filled(commands.to(DEV), dpoints.to(DEV), n, 1).cpu()
    want = GR.sample_points_bwd(commands, dpoints, n=n)
    assert (got - want).abs().max().item() <= n * 2.0 ** -22 * 14
    assert torch.equal(got, ops.sample_points_bwd(commands.to(DEV), dpoints.to(DEV), n=n).cpu())
    z = torch.arange(n - 1, dtype=torch.float64) / (n - 1)
    dp = dpoints.double()
    # the m row before the first drawing row gets the start point's share of that row: sum (1 - z) dP over the line's samples
    m_share = ((1 - z).unsqueeze(1) * dp[1, :n - 1]).sum(0)
    assert (got[1, 1, 9:11].double() - m_share).abs().max().item() <= 1e-5 and float(got[1, 1, 9:11].abs().min()) > 0
    assert torch.equal(got[1, 0], torch.zeros(11)) and torch.equal(got[1, 4:], torch.zeros(2, 11))
    assert torch.equal(got[2], torch.zeros(6, 11))
    # row 0's line: its end position receives sum z dP of its own samples + the curve's start share; nothing receives the
    # line's start share, so the row's total falls short of the total of dP by exactly sum (1 - z) dP of the line
    line_start = ((1 - z).unsqueeze(1) * dp[0, :n - 1]).sum(0)
    total = got[0].double().sum(0)
    assert (total[5:7] + total[7:9] + total[9:11] + line_start - dp[0, :2 * (n - 1) + 1].sum(0)).abs().max().item() <= 1e-4


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(gpu_device):
    c = torch.zeros(2, 4, device=DEV)
    for n in (1, 65):
        with pytest.raises(lib.DsvgError, match="2..64"):
            ops.sample_points_bwd(c, torch.zeros(2, 4 * (n - 1) + 1, 2, device=DEV), n=n)
    with pytest.raises(lib.DsvgError, match="tokens per cloud"):
        ops.sample_points_bwd(torch.zeros(1, 2049, device=DEV), torch.zeros(1, 2049 * 9 + 1, 2, device=DEV))
    with pytest.raises(lib.DsvgError):
        ops.sample_points_bwd(c.cpu(), torch.zeros(2, 37, 2))
    with pytest.raises(AssertionError, match="float32 commands"):
        ops.sample_points_bwd(c.long(), torch.zeros(2, 37, 2, device=DEV))
    p, k = torch.zeros(2, 5, 2, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
    with pytest.raises(lib.DsvgError):
        ops.chamfer_nn(p.cpu(), k.cpu(), p.cpu(), k.cpu())
    with pytest.raises(lib.DsvgError):
        ops.chamfer_bwd(p, k, p, k, torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32), torch.ones(2))
    L = lib.load()
    q = p.data_ptr()
    assert L.dsvg_sample_points_bwd(None, 2, 1, 4, 10, q, q, None) != 0 and b"null" in L.dsvg_last_error()
    assert L.dsvg_chamfer_nn(q, q, 5, q, q, 5, 2, q, None, q, q, 64, None) != 0 and b"null" in L.dsvg_last_error()
    assert L.dsvg_chamfer_nn(q, q, 5, q, q, 5, 2, q, q, q, q, 8, None) != 0 and b"workspace" in L.dsvg_last_error()
    assert L.dsvg_chamfer_nn(q, q, 0, q, q, 5, 2, q, q, q, q, 64, None) != 0 and b"bad shape" in L.dsvg_last_error()
    assert L.dsvg_chamfer_bwd(q, q, 5, q, q, 5, 2, q, q, None, q, q, None) != 0 and b"null" in L.dsvg_last_error()
    assert L.dsvg_chamfer_bwd(q, q, 5, q, q, 5, 0, q, q, q, q, q, None) != 0 and b"bad shape" in L.dsvg_last_error()


# ---- chamfer_loss / refine ------------------------------------------------------------------------------------------------
def test_chamfer_loss_masks_the_empty_icon(gpu_device):
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    cx = commands[i].clone()
    cx[1] = torch.where((cx[1] == 1) | (cx[1] == 2), torch.zeros(()), cx[1])
    with torch.no_grad():
        ty, tn = metrics.sample_points(commands[j].to(DEV), args[j].to(DEV), N)
    a = args[i].to(DEV).requires_grad_(True)
    res = metrics.chamfer_loss(cx.to(DEV), a, ty, tn, N)
    assert res["valid"].tolist() == [True, False, True, True, True, True] and torch.isfinite(res["loss"]).item()
    res["loss"].backward()
    assert bool(torch.isfinite(a.grad).all()) and torch.equal(a.grad[1].cpu(), torch.zeros(66, 11))
    assert float(a.grad[0].abs().max()) > 0


def test_refine_on_the_device(gpu_device):
    g, commands, args, pairs = golden_grad()
    i, j = pairs.unbind(1)
    with torch.no_grad():
        ty, tn = metrics.sample_points(commands[j].to(DEV), args[j].to(DEV), N)
    before = args[i].to(DEV)
    refined, history = metrics.refine(commands[i].to(DEV), before, ty, tn, steps=20, lr=0.1, n=N)
    assert history.is_cuda and history.shape == (20,)
    h = history.cpu()
    print(f"refine, 20 steps of Adam (lr 0.1) on the six golden pairs: loss {h[0].item():.4f} -> {h[-1].item():.4f}")
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(refined).all())
    assert h[-1].item() < h[0].item()
    assert torch.equal(refined[:, :, :5], before[:, :, :5]), "columns 0-4 moved"
    lens = torch.from_numpy(np.asarray(dict(np.load(GOLDEN_POINTS))["lens"]))[i].long()
    pad = (torch.arange(commands.shape[1]).unsqueeze(0) >= lens.unsqueeze(1)).to(DEV)
    assert torch.equal(refined[pad], before[pad]), "padding rows moved"
    assert not torch.equal(refined, before)
