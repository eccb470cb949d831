"""deepsvg_amd.paths.overlap / compute_filling on the device (csrc/paths_fill.hip) against the float64 restatement
(tests/paths_fill_ref.py), which is fed the device's own chord records.

Bounds.  With `l`-only icons, integer arguments, n = 2 and 256 or 64 samples every vertex, every sample coordinate (k + 0.5
or 4 k + 2) and every product of the sign test is exact in float32, so the counts equal the restatement's exactly.  With
curves the float32 sign test may differ from the float64 one on BORDERLINE samples only (tests/paths_fill_ref.py: 0 < |e| <=
2**-20 (|dx py| + |dy px|), sixteen times the rounding of the device's expression), so every count is within the number of
samples that are borderline for one of its two groups; tests/test_paths_fill_host.py shows they are below 1 % of an icon.
Everything behind the counts is integer and float64 work on them: equality.

Samples that lie EXACTLY on a chord (e == 0 in float64: an end position or a chord's midpoint of an int64 icon under an integer
sample centre, at 64 and 128 samples) are not borderline and count no crossing on either side: the counts kernel takes the
sweeps' sign test e = fmaf(dx, py, -(dy * px)) with the rounding residual of dy * px taken out (chord_side<true>,
csrc/svg_seq.h).  (With the sweeps' form as it is the device returned that residual there, and four int64 cases were 1-2
samples past the bound; the test still prints the count of such samples next to every figure.)  The sweeps keep their
form, so at such a pixel the rasteriser may take the other side - where its ink is 0.5 -+ d / s with d zero up to rounding;
test_area_lies_between_the_rasterisers_strict_and_weak_inside is the check that this stays inside the issue's bracket."""
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import ops, paths, render
from tests import paths_fill_ref as FR
from tests.poison import three_runs
from tests.test_draw_host import _check_ring, ring
from tests.test_paths_fill_host import CURVE_SAMPLES, CURVE_SHAPES, curve_icons
from tests.test_render_host import square

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTLINE, FILL, ERASE = FR.OUTLINE, FR.FILL, FR.ERASE
KEYS = ("filling", "depth", "parent", "clockwise", "paint_order", "area", "inter")


def device_records(commands, args, n):
    N, G, S = commands.shape
    modes = torch.ones(N, G, dtype=torch.int32, device=commands.device)
    return ops.raster_segments_layers(commands.reshape(N * G, S).contiguous(), args.reshape(N * G, S, 11).contiguous(), modes,
                                      n=n, groups=G)


def counts_and_restatement(commands, args, samples, n, evenodd=False, with_on_line=False):
    """-> device (area, inter) as numpy, and the restatement's (area, inter, borderline) on the device's records"""
    got = paths.overlap(commands, args, samples=samples, n=n, evenodd=evenodd)
    assert got["area"].dtype == torch.int32 and got["inter"].dtype == torch.int32 and got["fraction"].dtype == torch.float32
    segs, seg_counts, layer_first = device_records(commands, args, n)
    want = FR.overlap_counts(segs.cpu().numpy(), seg_counts.cpu().numpy(), layer_first.cpu().numpy(), samples, evenodd,
                             with_on_line=with_on_line)
    area, inter = got["area"].cpu().numpy().astype(np.int64), got["inter"].cpu().numpy().astype(np.int64)
    assert np.array_equal(inter, inter.transpose(0, 2, 1)), "inter is not symmetric"
    assert np.array_equal(np.diagonal(inter, axis1=1, axis2=2), area), "the diagonal of inter is not area"
    frac = np.where(area[:, :, None] > 0, inter / np.maximum(area[:, :, None], 1), 0.0).astype(np.float32)
    assert np.allclose(got["fraction"].cpu().numpy(), frac, rtol=2e-7, atol=0)
    return area, inter, want


def line_icons(N, G, S, seed, empty=(), full_rows=None):
    """`l`-only icons with integer arguments: every group is m, l ... l, EOS ...; `empty`: (icon, group) pairs left without
    commands; full_rows: {(icon, group): number of l rows}, otherwise random in 2..S - 1"""
    gen = torch.Generator().manual_seed(seed)
    commands = torch.full((N, G, S), 4, dtype=torch.int64)
    args = torch.randint(0, 256, (N, G, S, 11), generator=gen)
    for b in range(N):
        for g in range(G):
            if (b, g) in empty:
                continue
            rows = (full_rows or {}).get((b, g), int(torch.randint(2, S, (1,), generator=gen)))
            commands[b, g, 0] = 0
            commands[b, g, 1:1 + rows] = 1
    return commands, args


EXACT_CASES = {
    "3x1x6": dict(N=3, G=1, S=6, seed=1),
    "2x8x12": dict(N=2, G=8, S=12, seed=2, empty={(0, 0), (0, 3), (0, 7), (1, 0), (1, 1), (1, 4), (1, 5), (1, 6), (1, 7)}),
    "1x32x8": dict(N=1, G=32, S=8, seed=3, empty={(0, 0), (0, 13), (0, 14), (0, 31)}),
    # group 0: 511 `l` and the closing chord = 512 records, one LDS tile exactly
    "1x2x600": dict(N=1, G=2, S=600, seed=4, full_rows={(0, 0): 511, (0, 1): 40}),
}


@pytest.mark.parametrize("dtype", [torch.int64, torch.float32])
@pytest.mark.parametrize("samples", [256, 64])
@pytest.mark.parametrize("case", sorted(EXACT_CASES))
def test_counts_are_exact_on_line_icons(gpu_device, case, samples, dtype):
    commands, args = line_icons(**EXACT_CASES[case])
    commands, args = commands.to(gpu_device, dtype), args.to(gpu_device, dtype)
    area, inter, (want_area, want_inter, border) = counts_and_restatement(commands, args, samples, n=2)
    if case == "1x2x600":
        _, _, layer_first = device_records(commands, args, 2)
        assert layer_first.cpu().tolist() == [[0, 512, 553]]
    diff = int(np.abs(inter - want_inter).max())
    print(f"{case} samples={samples} {dtype}: worst count difference {diff}; borderline samples {int(border.max())}; "
          f"samples inside a group {int(area.sum())}, inside two {int((inter.sum() - area.sum()) // 2)}")
    assert diff == 0 and np.array_equal(area, want_area)
    assert area.sum() > 0 and (area.shape[1] == 1 or inter.sum() > area.sum())
    for b, g in EXACT_CASES[case].get("empty", ()):
        assert area[b, g] == 0 and not inter[b, g].any() and not inter[b, :, g].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("samples", CURVE_SAMPLES)
@pytest.mark.parametrize("shape", CURVE_SHAPES)
def test_counts_on_curves_differ_by_borderline_samples_at_most(gpu_device, shape, samples, dtype):
    B, G, L, seed = shape
    commands, args = (t.to(gpu_device) for t in curve_icons(B, G, L, seed, dtype))
    worst = []
    for evenodd in (False, True):
        area, inter, (want_area, want_inter, border, on_line) = counts_and_restatement(commands, args, samples, n=10,
                                                                                      evenodd=evenodd, with_on_line=True)
        diff = np.abs(inter - want_inter)
        worst.append(int((diff - border).max()))
        print(f"{shape} samples={samples} {dtype} evenodd={evenodd}: worst |device - restatement| {int(diff.max())}, worst "
              f"excess over the borderline count {worst[-1]} (entries in excess: {int((diff > border).sum())}), over borderline "
              f"+ exactly-on-a-line samples {int((diff - border - on_line).max())}; borderline at most {int(border.max())}, on a "
              f"line at most {int(on_line.max())}; samples inside a group {int(area.sum())}")
        assert area.sum() > 0
    assert max(worst) <= 0


@pytest.mark.parametrize("shape", [CURVE_SHAPES[0], CURVE_SHAPES[2]])       # one LDS tile per icon, and several
def test_area_lies_between_the_rasterisers_strict_and_weak_inside(gpu_device, shape):
    B, G, L, seed = shape
    samples = 64
    for dtype in (torch.float32, torch.int64):
        commands, args = (t.to(gpu_device) for t in curve_icons(B, G, L, seed, dtype))
        area = paths.overlap(commands, args, samples=samples)["area"].cpu()
        for g in range(G):
            ink = ops.rasterize(commands[:, g].contiguous(), args[:, g].contiguous(), size=samples, fill=True).cpu()
            lo, hi = (ink > 0.5).sum((1, 2)), (ink >= 0.5).sum((1, 2))
            print(f"{dtype} group {g}: #(ink > 0.5) {lo.tolist()} <= area {area[:, g].tolist()} <= #(ink >= 0.5) {hi.tolist()}")
            assert bool((lo <= area[:, g]).all()) and bool((area[:, g] <= hi).all())


@pytest.mark.parametrize("shape,samples", [(CURVE_SHAPES[0], 33), (CURVE_SHAPES[2], 64)])
def test_results_do_not_depend_on_uninitialised_memory_or_on_the_run(gpu_device, shape, samples):
    B, G, L, seed = shape
    commands, args = (t.to(gpu_device) for t in curve_icons(B, G, L, seed, torch.float32))
    runs = three_runs(lambda: paths.compute_filling(commands, args, samples=samples)) + [paths.compute_filling(commands, args, samples=samples)]
    for other in runs[1:]:
        for k in KEYS:
            assert torch.equal(runs[0][k], other[k]), k
    assert bool((runs[0]["filling"] != OUTLINE).any())


@pytest.mark.parametrize("rule", ["evenodd", "orientation"])
def test_filling_from_counts_equals_the_restatement_on_the_golden_graphs(gpu_device, rule):
    g = np.load(os.path.join(ROOT, "tests", "golden", "paths", "filling.npz"))
    adj = (g["adj"][:, :, None] >> np.arange(8, dtype=np.uint8)[None, None, :]) & 1
    N = adj.shape[0]
    (c, a), (cr, ar) = square(length=6), square(reverse=True, length=6)
    cw = torch.from_numpy(g["clockwise"])
    commands = torch.where(cw[:, :, None], c[0], cr[0]).contiguous()
    args = torch.where(cw[:, :, None, None], a[0], ar[0]).contiguous()
    counts = [FR.counts_from_adjacency(adj[k]) for k in range(N)]
    area, inter = np.stack([v[0] for v in counts]), np.stack([v[1] for v in counts])
    closed = torch.ones(N, 8, dtype=torch.bool)
    closed[::5, 2] = False                              # and some groups that do not participate
    got = ops.filling_from_counts(torch.from_numpy(area).to(gpu_device), torch.from_numpy(inter).to(gpu_device),
                                  commands.to(gpu_device), args.to(gpu_device), closed.to(gpu_device), threshold=0.9, rule=rule)
    got = {key: v.cpu() for key, v in got.items()}
    assert torch.equal(got["clockwise"], cw)
    wrong = 0
    for k in range(N):
        want = FR.filling_from_counts(area[k], inter[k], g["clockwise"][k], closed[k].tolist(), 0.9, rule)
        wrong += any(got[key][k].tolist() != want[key] for key in ("filling", "depth", "parent", "paint_order"))
        if rule == "orientation" and g["order_free"][k] and bool(closed[k].all()):
            assert got["filling"][k].tolist() == g["filling"][k].tolist(), "the reference's own walk"
    print(f"rule={rule}: {wrong} of {N} icons differ from the restatement")
    assert wrong == 0
    assert got["filling"].dtype == torch.int64 and got["paint_order"].dtype == torch.int64
    assert got["depth"].dtype == torch.int32 and got["parent"].dtype == torch.int32 and got["clockwise"].dtype == torch.bool


def test_whole_op_equals_the_restatement(gpu_device):
    B, G, L, seed = CURVE_SHAPES[0]
    commands, args = (t.to(gpu_device) for t in curve_icons(B, G, L, seed, torch.int64))
    closed = torch.ones(B, G, dtype=torch.bool, device=gpu_device)
    closed[0, 1] = False
    for rule, threshold in (("evenodd", 0.9), ("orientation", 0.5)):
        got = paths.compute_filling(commands, args, rule=rule, threshold=threshold, samples=64, closed=closed)
        for b in range(B):
            cw = [FR.is_clockwise(commands[b, g].cpu(), args[b, g].cpu()) for g in range(G)]
            want = FR.filling_from_counts(got["area"][b].cpu().numpy(), got["inter"][b].cpu().numpy(), cw,
                                          closed[b].cpu().tolist(), threshold, rule)
            assert got["clockwise"][b].cpu().tolist() == cw
            for key, v in want.items():
                assert got[key][b].cpu().tolist() == v, (rule, b, key)
    # (N, S) is read as G = 1, inputs are detached
    one = paths.compute_filling(commands[:, 0].float(), args[:, 0].float().requires_grad_(True), samples=64)
    assert one["filling"].shape == (B, 1) and not one["filling"].requires_grad


def test_swapped_ring_end_to_end(gpu_device):
    """the ring of tests/test_draw_host.py with its groups in the wrong paint order and no filling given: compute_filling finds
    the hole and the order, and render.draw paints the ring"""
    commands, args = (t.flip(1).contiguous().to(gpu_device) for t in ring())
    r = paths.compute_filling(commands, args, rule="evenodd")
    print("swapped ring:", {k: r[k].cpu().tolist() for k in KEYS})
    assert r["filling"].cpu().tolist() == [[ERASE, FILL]] and r["depth"].cpu().tolist() == [[1, 0]]
    assert r["parent"].cpu().tolist() == [[1, -1]] and r["paint_order"].cpu().tolist() == [[1, 0]]
    assert r["clockwise"].cpu().tolist() == [[True, True]]
    order = r["paint_order"]
    c = torch.gather(commands, 1, order[:, :, None].expand_as(commands))
    a = torch.gather(args, 1, order[:, :, None, None].expand_as(args))
    f = torch.gather(r["filling"], 1, order)
    _check_ring(render.draw(c, a, filling=f, size=64)[0].cpu())
    with pytest.raises(AssertionError):
        _check_ring(render.draw(commands, args, filling=r["filling"], size=64)[0].cpu())
    assert paths.compute_filling(commands, args, rule="orientation")["filling"].cpu().tolist() == [[FILL, FILL]]
