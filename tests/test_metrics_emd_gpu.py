"""The ordered point loss and the polyline length on a real MI355X: dsvg_emd, dsvg_emd_bwd, dsvg_polyline_length and
dsvg_polyline_length_bwd (csrc/metrics.hip) against the reference's own results (tests/golden/metrics/metrics_emd.npz) and
the float64 restatements of tests/emd_ref.py, stage by stage, their exactness properties on integer coordinates, and
emd_loss / refine(loss="emd") end to end.  Every test prints the largest error it saw before it asserts.

Bounds (EPS = 2^-24, half an fp32 ulp of 1):
  end to end        the loss within CHAMFER_ATOL, the gradient within 4 x ref_spread of the fixture, matched and shift equal
  matching          float64 on both sides: a matched index is valid when its |u_i - D_j| is within 1e-9 of the float64 minimum
                    (the kernel adds the segment lengths chunk by chunk, the restatement in one cumsum: 1e-16 relative each)
  shift             S(s) of the `float_terms` restatement FED THE KERNEL'S OWN t: the kernel's shift is its arg-min wherever
                    its best and second-best differ by more than 2^-20 S, and S(kernel's shift) <= min S + 2^-20 S always
                    (a term differs by one rounding of the sum of squares, fused on the device: 2^-24 relative on S; the
                    inputs are seeded so that no case comes that close, which the test asserts on the CPU side)
  loss              given t and the shift, 8 EPS loss: per term one fp32 subtraction rounding per coordinate (EPS relative on
                    each, so at most EPS on the distance), one rounding of the sum of squares (EPS / 2 on the distance) and
                    one of the sqrt (EPS): 2.5 EPS per term, relative, hence on the float64 sum; the restatement's own terms
                    carry as much (5 EPS together), and the final fp32 rounding of loss adds EPS: 6 EPS, bound 8 EPS
  emd_bwd           a unit vector over n from the same fp32 differences, a product with sqrt(d2) * n and a division: a few
                    roundings of a value <= w_k / n: 8 EPS w_k / n per element at dout = 1
  polyline_length   float64 segment lengths and sums on the device, one fp32 rounding at the end: 4 EPS L
  its backward      two unit vectors from fp32 differences: 8 EPS per element at dout = 1
"""
import numpy as np
import pytest
import torch

from deepsvg_amd import lib, metrics, ops
from tests import emd_ref as ER
from tests.test_metrics_emd_host import N, golden_emd, grad_bound
from tests.test_metrics_gpu import _random_sequences
from tests.test_metrics_host import CHAMFER_ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _bits(t):
    return t.view(torch.int32)


# ---- end to end against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_emd_loss_matches_the_reference(gpu_device, weighted):
    g, cx, ax, cy, ay = golden_emd()
    sfx = "_w" if weighted else ""
    with torch.no_grad():
        ty, tn = metrics.sample_points(cy.to(DEV), ay.to(DEV), N)
    a = ax.to(DEV).requires_grad_(True)
    res = metrics.emd_loss(cx.to(DEV), a, ty, tn, N, first_point_weight=weighted)
    res["loss"].backward()
    el = (res["per_icon"].detach().cpu().double() - torch.from_numpy(g["loss" + sfx])).abs().max().item()
    eg = (a.grad.cpu().double() * len(tn) - torch.from_numpy(g["grad" + sfx])).abs().max().item()      # loss is the mean
    print(f"emd_loss per icon vs the reference (weight {weighted}): max abs err {el:.3e} (bound {CHAMFER_ATOL:.1e}); d / d args "
          f"err {eg:.3e} (bound {grad_bound(g):.3e}, ref_spread {float(g['ref_spread']):.3e})")
    assert bool(res["valid"].all())
    px, nx = metrics.sample_points(cx.to(DEV), a, N)
    loss, matched, shift = metrics.emd(px, nx, ty, tn, first_point_weight=weighted, return_matched_indices=True)
    assert loss.requires_grad and torch.equal(_bits(loss.detach()), _bits(res["per_icon"].detach()))
    assert torch.equal(matched.cpu(), torch.from_numpy(g["matched"])), "matched indices differ from the reference's"
    assert torch.equal(shift.cpu(), torch.from_numpy(g["shift"]))
    assert el <= CHAMFER_ATOL
    assert eg <= grad_bound(g)
    with torch.no_grad():                               # the differentiable call has the forward-only call's bits
        again = metrics.emd(px, nx, ty, tn, first_point_weight=weighted)
    assert torch.equal(_bits(again), _bits(loss.detach())) and not again.requires_grad


# ---- stage by stage ---------------------------------------------------------------------------------------------------------
# (n, m): the 64-lane wave, the 256-shift block, more than one block, the 1,024-point chunks and tiles, single points, both empties
BATCHES = [[(1, 2), (2, 2), (63, 65)],
           [(64, 64), (65, 1), (255, 257)],
           [(256, 256), (257, 1023), (1025, 3)],
           [(0, 5), (5, 0), (4096, 300)],
           [(300, 1024), (7, 1025), (600, 2500)]]      # (not in the issue's list: targets of one full chunk, and of more)


@pytest.fixture(scope="module")
def stage_runs(gpu_device):
    """per batch and weight: the clouds (caps unequal and larger than every count, NaN past the counts), the kernel's
    outputs on the host and, computed once, the `float_terms` restatement's S(s) fed the kernel's t"""
    gen = torch.Generator().manual_seed(5)
    runs = []
    for sizes in BATCHES:
        capx, capy = max(s[0] for s in sizes) + 5, max(s[1] for s in sizes) + 2
        px, py = torch.rand(3, capx, 2, generator=gen) * 255, torch.rand(3, capy, 2, generator=gen) * 255
        nx = torch.tensor([s[0] for s in sizes], dtype=torch.int32)
        ny = torch.tensor([s[1] for s in sizes], dtype=torch.int32)
        for b, (n, m) in enumerate(sizes):
            px[b, n:], py[b, m:] = float("nan"), float("nan")          # rows past the counts must never be read
        dpx, dnx, dpy, dny = _dev(px, nx, py, ny)
        out, shift, matched, t = ops.emd(dpx, dnx, dpy, dny, False)
        out_w, shift_w, matched_w, t_w = ops.emd(dpx, dnx, dpy, dny, True)
        dout = torch.ones(3, device=DEV)
        grad, grad_w = ops.emd_bwd(dpx, dnx, dny, t, shift, dout, False), ops.emd_bwd(dpx, dnx, dny, t, shift, dout, True)
        torch.cuda.synchronize()
        assert torch.equal(shift, shift_w) and torch.equal(matched, matched_w), "the weight moved the shift"
        live = (torch.arange(capx, device=DEV).unsqueeze(0) < dnx.unsqueeze(1)) & (dny > 0).unsqueeze(1)
        assert torch.equal(_bits(t[live]), _bits(t_w[live]))
        t = torch.where(live.unsqueeze(-1), t, torch.zeros_like(t)).cpu()          # rows past the counts hold anything
        S = [ER.shift_sums(px[b, :n], t[b, :n], float_terms=True) if n and m else None for b, (n, m) in enumerate(sizes)]
        runs.append(dict(px=px, nx=nx, py=py, ny=ny, out=out.cpu(), out_w=out_w.cpu(), shift=shift.cpu(), matched=matched.cpu(),
                         t=t, S=S, grad=grad.cpu(), grad_w=grad_w.cpu()))
    return runs


def test_matching_is_the_float64_arg_min(stage_runs):
    worst = 0.0
    for run, sizes in zip(stage_runs, BATCHES):
        for b, (n, m) in enumerate(sizes):
            mt = run["matched"][b]
            assert bool((mt[n:] == -1).all()), "matched past the count"
            if n == 0 or m == 0:
                assert bool((mt == -1).all()) and run["shift"][b].item() == 0
                continue
            assert bool(((mt[:n] >= 0) & (mt[:n] < m)).all()), "matched index outside the target"
            s = int(run["shift"][b])
            match = torch.cat([mt[n - s:n], mt[:n - s]]).long()          # matched[k] = match[(k + s) mod n]
            assert torch.equal(run["t"][b, :n], run["py"][b, :m][match]), "t is not the target at the matched indices"
            worst = max(worst, ER.match_error(n, run["py"][b, :m], match).max().item())
    print(f"matching: |u_i - D_j| of the chosen j - float64 minimum, largest {worst:.3e} (bound 1e-9)")
    assert worst <= 1e-9


def test_shift_is_the_arg_min_of_the_float64_sums(stage_runs):
    worst, closest = 0.0, float("inf")
    for run, sizes in zip(stage_runs, BATCHES):
        for b, (n, m) in enumerate(sizes):
            if n == 0 or m == 0:
                continue
            S, s = run["S"][b], int(run["shift"][b])
            assert 0 <= s < n
            tol = 2.0 ** -20 * S.min().item()
            if n > 1 and m > 1:                                           # (one target point: every shift is the same sum)
                two = S.topk(2, largest=False).values
                closest = min(closest, (two[1] - two[0]).item() / max(tol, 1e-300))
                assert (two[1] - two[0]).item() > tol, f"(n, m) = ({n}, {m}): the seeded input has a near-tie of shifts"
                assert s == int(S.argmin()), f"(n, m) = ({n}, {m}): shift {s}, the restatement's {int(S.argmin())}"
            else:
                assert s == 0, "equal sums: the lowest shift"
            worst = max(worst, (S[s] - S.min()).item() / max(tol, 1e-300))
    print(f"shift: S(kernel's shift) - min S, largest {worst:.3e} of the 2^-20 S allowance; the closest second-best shift is "
          f"{closest:.3e} allowances away")
    assert worst <= 1.0


def test_loss_given_t_and_shift(stage_runs):
    worst = 0.0
    for run, sizes in zip(stage_runs, BATCHES):
        for b, (n, m) in enumerate(sizes):
            if n == 0:
                assert run["out"][b].item() == 0.0 and run["out_w"][b].item() == 0.0
                continue
            if m == 0:
                assert torch.isnan(run["out"][b]).item() and torch.isnan(run["out_w"][b]).item()
                continue
            s = int(run["shift"][b])
            first = ER.terms(run["px"][b, 0], run["t"][b, s], True).item()
            for key, want in (("out", run["S"][b][s].item() / n), ("out_w", (run["S"][b][s].item() + 9.0 * first) / n)):
                worst = max(worst, abs(run[key][b].item() - want) / (8 * EPS * want))
    print(f"loss given t and shift: largest error {worst:.3f} of the 8 EPS loss bound")
    assert worst <= 1.0


def test_emd_bwd_matches_the_restatement(stage_runs):
    worst = 0.0
    for run, sizes in zip(stage_runs, BATCHES):
        for key, weighted in (("grad", False), ("grad_w", True)):
            want = ER.emd_bwd(run["px"], run["nx"], run["ny"], run["t"], run["shift"], torch.ones(3), weighted, as_double=True)
            got = run[key]
            assert bool(torch.isfinite(got).all()), "a row past the counts or of an empty icon is not zero"
            for b, (n, m) in enumerate(sizes):
                if n == 0 or m == 0:
                    assert torch.equal(got[b], torch.zeros_like(got[b]))
                    continue
                assert torch.equal(got[b, n:], torch.zeros_like(got[b, n:]))
                w = torch.ones(n, 1, dtype=torch.float64)
                w[0] = 10.0 if weighted else 1.0
                worst = max(worst, ((got[b, :n].double() - want[b, :n]).abs() / (8 * EPS * w / n)).max().item())
    print(f"emd_bwd: largest error {worst:.3f} of the 8 EPS w_k / n bound")
    assert worst <= 1.0


def test_polyline_length_and_its_backward(stage_runs):
    worst, worst_b = 0.0, 0.0
    for run in stage_runs:
        for p, c in ((run["px"], run["nx"]), (run["py"], run["ny"])):
            dp, dc = _dev(p, c)
            got = ops.polyline_length(dp, dc)
            assert torch.equal(_bits(got), _bits(ops.polyline_length(dp, dc))), "not reproducible"
            want = ER.polyline_length(p, c, as_double=True)
            got = got.cpu().double()
            short = c < 2
            assert torch.equal(got[short], torch.zeros_like(got[short]))
            worst = max(worst, ((got - want).abs() / (4 * EPS * want).clamp(min=1e-300))[~short].max().item())
            gb = ops.polyline_length_bwd(dp, dc, torch.ones(len(c), device=DEV)).cpu()
            assert bool(torch.isfinite(gb).all()), "a row past the counts is not zero"
            worst_b = max(worst_b, (gb.double() - ER.polyline_length_bwd(p, c, torch.ones(len(c)), as_double=True)).abs().max().item())
    print(f"polyline_length: largest error {worst:.3f} of the 4 EPS L bound; backward: {worst_b:.3e} (bound {8 * EPS:.3e})")
    assert worst <= 1.0 and worst_b <= 8 * EPS


# ---- exactness on integer coordinates -------------------------------------------------------------------------------------------
def _square_lap(side=75):
    """the boundary of a square in unit steps, 4 * side points, every segment (the closing one included) of length 1;
    shoelace sum > 0: kept as it is by the orientation rule"""
    k = torch.arange(side, dtype=torch.float32)
    z, s = torch.zeros(side), torch.full((side,), float(side))
    return torch.cat([torch.stack([k, z], 1), torch.stack([s, k], 1), torch.stack([s - k, s], 1), torch.stack([z, s - k], 1)])


def _one(x, y, weighted=False, capx=None, capy=None):
    """one icon through ops.emd and ops.emd_bwd -> out, shift, matched[:n], grad[:n], on the host"""
    n, m = len(x), len(y)
    px = torch.full((1, capx or n + 3, 2), float("nan"))
    py = torch.full((1, capy or m + 1, 2), float("nan"))
    px[0, :n], py[0, :m] = x, y
    nx, ny = torch.tensor([n], dtype=torch.int32), torch.tensor([m], dtype=torch.int32)
    dpx, dnx, dpy, dny = _dev(px, nx, py, ny)
    out, shift, matched, t = ops.emd(dpx, dnx, dpy, dny, weighted)
    grad = ops.emd_bwd(dpx, dnx, dny, t, shift, torch.ones(1, device=DEV), weighted)
    return out.cpu()[0], int(shift.cpu()[0]), matched.cpu()[0, :n], grad.cpu()[0, :n], t.cpu()[0, :n]


def _noisy_lap(seed):
    lap = _square_lap()
    noise = torch.randint(-4, 5, lap.shape, generator=torch.Generator().manual_seed(seed)).float()
    return lap, (lap.roll(-37, 0) + noise)


def test_periodic_tie_takes_the_lower_shift(gpu_device):
    """two laps of a unit-step square against a pred of period n / 2: D_j = j / 599 = u_j, so t is the target in order and
    periodic too; S(s) = S(s + 300) term by term, exact in float64: the tie is exact and crosses two 256-shift blocks"""
    lap, h = _noisy_lap(1)
    x, y = torch.cat([h, h]), torch.cat([lap, lap])
    out, shift, matched, _, t = _one(x, y)
    assert torch.equal(t, y), "the gathered target is not the target in order"
    S = ER.shift_sums(x, t, float_terms=True)
    want = int(S.argmin())
    assert want < 300 and S[want].item() == S[want + 300].item(), "the input does not tie"
    print(f"periodic tie: shift {shift}, the restatement's lowest {want} (tied with {want + 300}), loss {out.item():.6f}")
    assert shift == want
    assert out.item() == np.float32(S[want].item() / 600)
    out2, shift2, matched2, _, _ = _one(x, y)
    assert shift2 == shift and torch.equal(matched2, matched) and torch.equal(_bits(out2), _bits(out))


def test_self_match_is_exactly_zero(gpu_device):
    lap = _square_lap()
    out, shift, matched, grad, _ = _one(lap, lap)
    print(f"emd(x, x): loss {out.item()}, shift {shift}, largest gradient entry {grad.abs().max().item()}")
    assert out.item() == 0.0 and shift == 0
    assert torch.equal(matched, torch.arange(300, dtype=torch.int32))
    assert torch.equal(grad, torch.zeros(300, 2))


def test_reversed_target_gives_the_same_loss(gpu_device):
    lap, x = _noisy_lap(2)
    out, shift, matched, grad, _ = _one(x, lap)
    out_r, shift_r, matched_r, grad_r, _ = _one(x, lap.flip(0))            # A < 0: read in reverse
    print(f"reversal: loss {out.item():.6f} / {out_r.item():.6f}, shift {shift} / {shift_r}")
    assert out.item() > 0 and torch.equal(_bits(out), _bits(out_r)) and shift == shift_r == 37
    assert torch.equal(matched_r, 299 - matched) and torch.equal(_bits(grad), _bits(grad_r))


def test_collinear_target_is_reversed_and_ties_go_to_the_lowest_index(gpu_device):
    """target (0,0), (128,0), (256,0): A == 0 exactly, so it is read in reverse, D = 0, 0.5, 1; n = 5: u = 0.25 ties between
    D_0 and D_1 and u = 0.75 between D_1 and D_2 of the ORIENTED order, the lower wins: oriented 0, 0, 1, 1, 2 = as passed
    2, 2, 1, 1, 0.  The pred is exactly those points, so only this matching gives loss 0 at shift 0."""
    y = torch.tensor([[0., 0.], [128., 0.], [256., 0.]])
    x = y[[2, 2, 1, 1, 0]]
    out, shift, matched, grad, t = _one(x, y)
    print(f"collinear: loss {out.item()}, shift {shift}, matched {matched.tolist()}")
    assert matched.tolist() == [2, 2, 1, 1, 0] and out.item() == 0.0 and shift == 0
    assert torch.equal(t, x) and torch.equal(grad, torch.zeros(5, 2))


def test_first_point_weight(gpu_device):
    lap, x = _noisy_lap(3)
    out, shift, matched, grad, t = _one(x, lap)
    out_w, shift_w, matched_w, grad_w, _ = _one(x, lap, weighted=True)
    first = ER.terms(x[0], t[shift], True).item()
    err = abs(out_w.item() * 300 - (out.item() * 300 + 9 * first))
    print(f"first_point_weight: loss {out.item():.6f} -> {out_w.item():.6f}, the first pair's distance {first:.6f}; "
          f"n (loss_w - loss) - 9 d_0 = {err:.3e}")
    assert shift_w == shift and torch.equal(matched_w, matched)
    assert first > 0 and err <= 8 * EPS * 300 * (out.item() + out_w.item())      # two losses, each within 8 EPS of its own
    assert torch.equal(_bits(grad_w[1:]), _bits(grad[1:]))
    assert (grad_w[0].double() - 10 * grad[0].double()).abs().max().item() <= 2 * EPS * 10 * grad[0].abs().max().item()
    assert float(grad[0].abs().max()) > 0


# ---- limits and refusals ----------------------------------------------------------------------------------------------------
def test_a_pred_cloud_above_the_limit_is_refused(gpu_device):
    k = torch.ones(1, dtype=torch.int32, device=DEV)
    big, small = torch.zeros(1, 65537, 2, device=DEV), torch.zeros(1, 4, 2, device=DEV)
    with pytest.raises(lib.DsvgError, match="at most 65536 points"):
        ops.emd(big, k, small, k)
    with pytest.raises(lib.DsvgError, match="at most 65536 points"):
        ops.emd_bwd(big, k, k, big, k, torch.ones(1, device=DEV))
    ops.emd(small, k, big, k)                                             # the target may have any size
    with pytest.raises(lib.DsvgError):
        ops.emd(small.cpu(), k.cpu(), small.cpu(), k.cpu())
    with pytest.raises(lib.DsvgError):
        ops.polyline_length(small.cpu(), k.cpu())
    L = lib.load()
    q = small.data_ptr()
    assert L.dsvg_emd(q, q, 4, q, q, 4, 1, 0, q, q, q, q, q, 8, None) != 0 and b"workspace" in L.dsvg_last_error()
    assert L.dsvg_emd(q, q, 4, q, q, 4, 1, 0, q, q, q, None, q, 64, None) != 0 and b"null" in L.dsvg_last_error()
    assert L.dsvg_emd_bwd(q, q, 0, q, q, q, q, 0, 1, q, None) != 0 and b"bad shape" in L.dsvg_last_error()
    assert L.dsvg_polyline_length(q, q, 0, 1, q, None) != 0 and b"bad shape" in L.dsvg_last_error()
    assert L.dsvg_polyline_length_bwd(q, q, 4, 1, None, q, None) != 0 and b"null" in L.dsvg_last_error()
    assert L.dsvg_emd_workspace_bytes(2, 300) == 2 * 2 * 12 + 2 * 300 * 4


# ---- refine -------------------------------------------------------------------------------------------------------------------
def test_refine_with_the_ordered_loss_on_the_device(gpu_device):
    commands, args = _random_sequences(8, 1, 12, seed=21)
    commands, args = commands.reshape(8, 12).float(), args.reshape(8, 12, 11).float()
    noise = torch.rand(args.shape, generator=torch.Generator().manual_seed(22)) * 6 - 3
    with torch.no_grad():
        ty, tn = metrics.sample_points(commands.to(DEV), args.to(DEV), 10)
    before = (args + noise).to(DEV)
    refined, history = metrics.refine(commands.to(DEV), before, ty, tn, steps=40, lr=0.1, n=10, loss="emd")
    assert history.is_cuda and history.shape == (40,)
    h = history.cpu()
    with torch.no_grad():
        first = metrics.emd_loss(commands.to(DEV), before, ty, tn, 10)
        last = metrics.emd_loss(commands.to(DEV), refined, ty, tn, 10)
    valid = first["valid"].cpu()
    print(f"refine(loss='emd'), 40 steps of Adam (lr 0.1), {int(valid.sum())} valid icons of 8: batch loss {h[0].item():.4f} -> "
          f"{h[-1].item():.4f}; per icon {first['per_icon'].cpu()[valid].tolist()} -> {last['per_icon'].cpu()[valid].tolist()}")
    assert int(valid.sum()) >= 4 and bool(torch.isfinite(h).all()) and bool(torch.isfinite(refined).all())
    assert torch.equal(_bits(h[0]), _bits(first["loss"].cpu()))
    assert h[-1].item() < h[0].item()
    draw = (commands == 1) | (commands == 2)
    feeds = draw | torch.cat([draw[:, 1:], torch.zeros(8, 1, dtype=torch.bool)], 1)       # a row's end starts the next row
    assert torch.equal(refined[:, :, :5], before[:, :, :5]), "columns 0-4 moved"
    assert torch.equal(refined[(~feeds).to(DEV)], before[(~feeds).to(DEV)]), "rows that give no point moved"
    assert not torch.equal(refined, before)
