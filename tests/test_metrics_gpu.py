"""deepsvg_amd.metrics on a real MI355X: dsvg_sample_points and dsvg_chamfer (csrc/metrics.hip) against the reference's
golden and the float64 restatements of tests/metrics_ref.py, their exactness properties, and reconstruction_error end to
end.  Every test prints the largest error it saw before it asserts.

Tolerances (as in tests/test_metrics_host.py): points 5e-4 - a coefficient sum of the cubic reaches 8 * 255 ~ 2048, half an
fp32 ulp there is 1.2e-4, four such terms; Chamfer 1e-4 - a distance of at most 362 from fp32 differences carries a few
ulps.  Points are drawn from 0..255, the range of the arguments."""
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import lib, metrics, ops
from tests import helpers as H
from tests import metrics_ref as MR
from tests.test_metrics_host import CHAMFER_ATOL, POINT_ATOL, check_points_against_golden, golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 1024            # CH_TILE = CH_SLICE of csrc/metrics.hip: points of the streamed cloud per LDS tile, and of a workgroup's slice


def _as(t, dtype):
    return (t.long() if dtype == torch.int64 else t.float()).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [2, 7, 10])
def test_sample_points_match_the_reference_golden(gpu_device, n, dtype):
    g, commands, args = golden()
    points, counts = ops.sample_points(_as(commands, dtype), _as(args, dtype), n=n)
    assert points.shape == (commands.shape[0], commands.shape[1] * (n - 1) + 1, 2)
    worst = check_points_against_golden(g, n, points.cpu(), counts.cpu())
    print(f"sample_points vs reference golden n={n} {dtype}: max abs err {worst:.3e}")


def _random_sequences(B, G, L, seed):
    """commands from all seven ids (l and c half of the time), arguments from -1..255 in EVERY slot (a start point is the
    row before's end position whatever that row holds); with G = 8, empty groups in the middle and at the end of an icon"""
    gen = torch.Generator().manual_seed(seed)
    pool = torch.tensor([0, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6])
    commands = pool[torch.randint(0, len(pool), (B, G, L), generator=gen)]
    if G > 1:
        commands[:, 3] = 4
        commands[0, G - 1] = 4
        commands[B - 1, G - 2:] = 4
    args = torch.randint(-1, 256, (B, G, L, 11), generator=gen)
    return commands, args


def _check_against_restatement(commands, args, n, dtype):
    B, G, L = commands.shape
    c, a = _as(commands.reshape(B * G, L), dtype), _as(args.reshape(B * G, L, 11), dtype)
    points, counts = ops.sample_points(c, a, n=n, groups=G)
    want_p, want_c = MR.sample_points(c.cpu(), a.cpu(), n=n, groups=G)
    assert points.shape == want_p.shape and counts.dtype == torch.int32
    assert torch.equal(counts.cpu(), want_c), "counts differ"
    points = points.cpu()
    live = torch.arange(points.shape[1]).unsqueeze(0) < want_c.unsqueeze(1)          # rows past counts[b] hold anything
    err = torch.where(live.unsqueeze(-1), (points - want_p).abs(), torch.zeros_like(points))
    assert not bool(torch.isnan(err).any())
    return err.max().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [2, 7, 10, 64])
def test_sample_points_match_the_restatement(gpu_device, n, dtype):
    worst = 0.0
    for B in (1, 5):
        for G in (1, 8):
            for L in (1, 32, 66):
                commands, args = _random_sequences(B, G, L, seed=1000 * B + 100 * G + L + n)
                worst = max(worst, _check_against_restatement(commands, args, n, dtype))
    print(f"sample_points vs float64 restatement n={n} {dtype}: max abs err {worst:.3e}")
    assert worst <= POINT_ATOL


@pytest.mark.parametrize("G,L", [(8, 256), (2048, 1), (1, 2048)])
def test_sample_points_at_2048_tokens_per_cloud(gpu_device, G, L):
    commands, args = _random_sequences(2, G, L, seed=77)
    worst = _check_against_restatement(commands, args, 10, torch.float32)
    print(f"sample_points G={G} L={L}: max abs err {worst:.3e}")
    assert worst <= POINT_ATOL


def test_sample_points_of_empty_sequences(gpu_device):
    commands = torch.tensor([[5, 0, 6, 4, 4], [4, 4, 4, 4, 4], [5, 0, 1, 4, 4]], dtype=torch.float32, device=DEV)
    args = torch.randint(0, 256, (3, 5, 11), generator=torch.Generator().manual_seed(0)).float().to(DEV)
    p, c = metrics.sample_points(commands, args, n=10)
    assert c.tolist() == [0, 0, 10]
    got = metrics.chamfer(p, c, p[2:3].expand(3, -1, -1).contiguous(), c[2:3].expand(3).contiguous())
    assert torch.isnan(got[:2]).all() and got[2] == 0


def test_bad_arguments_are_refused(gpu_device):
    c, a = torch.zeros(2, 4, device=DEV), torch.zeros(2, 4, 11, device=DEV)
    for n in (1, 65):
        with pytest.raises(lib.DsvgError, match="2..64"):
            ops.sample_points(c, a, n=n)
    with pytest.raises(lib.DsvgError, match="tokens per cloud"):
        ops.sample_points(torch.zeros(1, 2049, device=DEV), torch.zeros(1, 2049, 11, device=DEV))
    with pytest.raises(lib.DsvgError):
        ops.sample_points(c.cpu(), a.cpu())
    L = lib.load()
    assert L.dsvg_sample_points(1, c.data_ptr(), a.data_ptr(), 2, 1, 4, 10, c.data_ptr(), c.data_ptr(), None) != 0
    assert b"itype" in L.dsvg_last_error()
    assert L.dsvg_chamfer(None, None, 1, None, None, 1, 1, None, None, 0, None) != 0 and b"null" in L.dsvg_last_error()
    assert L.dsvg_chamfer(*[c.data_ptr()] * 2, 1, *[c.data_ptr()] * 2, 1, 1, c.data_ptr(), c.data_ptr(), 8, None) != 0
    assert b"workspace" in L.dsvg_last_error() and L.dsvg_chamfer_workspace_bytes(3, 1025, 7) == 3 * 2 * 2 * 8


# ---- Chamfer ------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 300), (255, 257), (256, 256), (2401, 1999), (TILE - 1, TILE - 1), (TILE + 1, TILE + 1),
         (0, 5), (5, 0), (0, 0)]


@pytest.fixture(scope="module")
def clouds():
    """one batch with a different pair of counts per icon, and its float64 brute-force Chamfer distances (computed once)"""
    gen = torch.Generator().manual_seed(5)
    capx, capy = max(s[0] for s in SIZES), max(s[1] for s in SIZES) + 3
    px, py = torch.rand(len(SIZES), capx, 2, generator=gen) * 255, torch.rand(len(SIZES), capy, 2, generator=gen) * 255
    nx = torch.tensor([s[0] for s in SIZES], dtype=torch.int32)
    ny = torch.tensor([s[1] for s in SIZES], dtype=torch.int32)
    return px, nx, py, ny, MR.chamfer(px, nx, py, ny, as_double=True)


def test_chamfer_matches_float64_brute_force(gpu_device, clouds):
    px, nx, py, ny, want = clouds
    got = ops.chamfer(px.to(DEV), nx.to(DEV), py.to(DEV), ny.to(DEV)).cpu()
    empty = (nx == 0) | (ny == 0)
    assert torch.equal(torch.isnan(got), empty) and int(empty.sum()) == 3
    err = (got.double() - want)[~empty].abs()
    for s, e in zip([s for s in SIZES if s[0] and s[1]], err.tolist()):
        print(f"chamfer {s}: abs err {e:.3e}")
    assert err.max().item() <= CHAMFER_ATOL
    # one icon at a time: the same bits as in the batch
    for b in (1, 4):
        one = ops.chamfer(px[b:b + 1].to(DEV), nx[b:b + 1].to(DEV), py[b:b + 1].to(DEV), ny[b:b + 1].to(DEV)).cpu()
        assert torch.equal(one, got[b:b + 1])


def test_chamfer_is_exact_where_it_can_be(gpu_device, clouds):
    px, nx, py, ny, _ = (t.to(DEV) if t.dtype != torch.float64 else t for t in clouds)
    live = (nx > 0).cpu()
    same = ops.chamfer(px, nx, px.clone(), nx).cpu()
    assert torch.equal(same[live], torch.zeros(int(live.sum()))), "chamfer(x, x) != 0"
    xy, yx = ops.chamfer(px, nx, py, ny), ops.chamfer(py, ny, px, nx)
    assert torch.equal(xy.view(torch.int32), yx.view(torch.int32)), "chamfer(x, y) and chamfer(y, x) differ in bits"
    again = ops.chamfer(px, nx, py, ny)
    assert torch.equal(xy.view(torch.int32), again.view(torch.int32)), "two runs differ in bits"


def test_chamfer_builds_no_distance_matrix(gpu_device):
    gen = torch.Generator().manual_seed(6)
    px, py = (torch.rand(4, 2431, 2, generator=gen) * 255).to(DEV), (torch.rand(4, 2431, 2, generator=gen) * 255).to(DEV)
    nx = torch.tensor([2400, 2431, 2399, 2405], dtype=torch.int32, device=DEV)
    ny = torch.tensor([2431, 2390, 2400, 2411], dtype=torch.int32, device=DEV)
    ops.chamfer(px, nx, py, ny)                         # (code objects loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.chamfer(px, nx, py, ny)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"chamfer of 4 x ~2,400 points: peak allocation grew by {grown} bytes")
    assert grown < (1 << 20) and bool(torch.isfinite(out).all())         # one icon's matrix alone: 23 MB


# ---- reconstruction_error -------------------------------------------------------------------------------------------------
def _model(name):
    g, cfg, commands, args, _ = H.golden_setup(name)
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(H.weights_for(model, g["wseed"]))
    model.to(DEV)
    model.set_compute_dtype(torch.float32)
    return model, commands.to(DEV), args.to(DEV)


@pytest.mark.parametrize("name", ["hier_ordered_n5", "onestage50_n3"])
def test_reconstruction_error_matches_the_restatement(gpu_device, name):
    model, commands, args = _model(name)
    model.train()
    decoded = {}
    greedy = model.greedy_sample

    def spy(*a, **k):
        decoded["out"] = greedy(*a, **k)
        return decoded["out"]
    model.greedy_sample = spy
    res = metrics.reconstruction_error(model, commands, args)
    assert model.training
    cy, ay = (t.cpu() for t in decoded["out"])
    c, a = commands.cpu(), args.cpu()
    px, nx = MR.sample_points(cy.reshape(-1, cy.shape[-1]), ay.reshape(-1, *ay.shape[-2:]), 10, groups=cy.shape[1])
    py, ny = MR.sample_points(c.reshape(-1, c.shape[-1]), a.reshape(-1, *a.shape[-2:]), 10, groups=c.shape[1])
    want = MR.chamfer(px, nx, py, ny, as_double=True)
    valid = (nx > 0) & (ny > 0)
    re = res["re"].cpu()
    assert torch.equal(res["valid"].cpu(), valid) and torch.equal(torch.isnan(re), ~valid)
    if bool(valid.any()):
        err = (re.double() - want)[valid].abs().max().item()
        print(f"reconstruction_error {name}: re {re.tolist()}, max abs err {err:.3e}")
        assert err <= CHAMFER_ATOL
        assert abs(res["mean"].item() - want[valid].mean().item()) <= CHAMFER_ATOL
    else:
        print(f"reconstruction_error {name}: every decoded icon is empty")
        assert torch.isnan(res["mean"]).item()


@pytest.mark.parametrize("name", ["hier_ordered_n5", "onestage50_n3"])
def test_reconstruction_error_of_the_targets_is_zero(gpu_device, name):
    model, commands, args = _model(name)
    model.greedy_sample = lambda *a, **k: (commands.long(), args.long())
    res = metrics.reconstruction_error(model, commands, args)
    assert bool(res["valid"].all())
    assert torch.equal(res["re"].cpu(), torch.zeros(commands.shape[0])) and res["mean"].item() == 0
