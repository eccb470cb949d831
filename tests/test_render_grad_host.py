"""The gradient of deepsvg_amd.render on CPU: the float64 restatement of tests/raster_grad_ref.py against central
differences, against autograd through the chord builder and on cases whose gradient is known in closed form; then the host
logic of rasterize_with_grad / image_loss / refine_to_images with the raster ops replaced by the restatement.  Every test
prints the largest error it saw before it asserts.

Inputs of the finite-difference and spread tests (`outlines`): sequences of one `m` and 3-4 random `l` / `c` commands with
float arguments rand * 256, so that no sub-path is degenerate (a sub-path of one `l` is retraced by its closing chord and
ties every pixel) and nothing sits on a pixel centre.  Differences are taken with respect to the ARGUMENTS, which moves a
vertex that two chords share as one: moved on its own, a chord's endpoint ties with its neighbour and the loss has a kink.

fp32 spread (test_fp32_spread_of_the_backward): the restated backward run in fp32 against float64, on the inputs the GPU
tests use (`GRAD_CASES` of `grad_batch()`: the seeds were chosen so that the smallest distance of a live pixel to its chord
is >= 1e-2 - q / d is ill-conditioned near the chord, the spread grows as 1 / d):
  SPREAD = 1.2e-5 (of max |dout|; dsegs itself reaches 0.7), smallest live d 2.72e-2; the spread measured is 1.12e-5, at
  size 33, and 1.2e-6 at size 16.
  SEG_SPREAD = 1.6e-6 (of max |dsegs|): raster_segments_bwd with fp32 weights and sums on the GPU test's shapes ((G, L) up to
  (8, 256), n up to 64; the weights lie in [0, 1]); measured 1.51e-6.
The GPU tests allow the kernels 4 x these.

The end-to-end fixture of the GPU tests (`e2e_fixture()`, margins stated by test_fixture_margins): in float64 no pixel lies
within 1e-3 ink of a clamp, no live pixel has a chord that does not share a vertex with its nearest one within 1e-3 of it, and
no live pixel is closer than 1e-2 to its chord - so the float64 restatement with its OWN arg-min and its own image picks the
pixels and chords the fp32 kernels pick."""
import numpy as np
import pytest
import torch

from deepsvg_amd import lib, render
from tests import raster_grad_ref as RG
from tests import raster_ref as RR
from tests.test_render_host import EOS, M, L_, C_, sequence, square

SPREAD, SEG_SPREAD, MIN_LIVE_D = 1.2e-5, 1.6e-6, 1e-2
FD_H, FD_ATOL = 1e-6, 1e-6


@pytest.fixture
def grad_ops(emulated_ops):
    saved = RG.install()
    yield
    RG.restore(saved)


def outlines(B, seed, length=6):
    """B sequences of `m` + 3-4 random `l` / `c` -> commands f32 [B, length], args float64 [B, length, 11] = rand * 256 on the
    rows in use, -1 (padding) past them"""
    gen = torch.Generator().manual_seed(seed)
    commands = torch.full((B, length), float(EOS))
    args = torch.full((B, length, 11), -1.0, dtype=torch.float64)
    for b in range(B):
        k = 3 + int(torch.randint(0, 2, (1,), generator=gen))
        commands[b, 0] = M
        commands[b, 1:1 + k] = torch.randint(L_, C_ + 1, (k,), generator=gen).float()
        args[b, :1 + k] = torch.rand(1 + k, 11, generator=gen, dtype=torch.float64) * 256.0
    return commands, args


def grad_batch():
    """the float-argument batch of the spread test and of the GPU tests: 4 icons of 2 groups -> commands f32 [8, 6], args
    f32 [8, 6, 11], groups = 2, n = 4"""
    commands, args = outlines(8, seed=GRAD_SEED)
    return commands, args.float(), 2, 4


GRAD_SEED = 78
GRAD_CASES = [(16, False), (16, True), (33, False), (33, True)]         # (size, fill)


def forward64(commands, args, size, fill, n, groups=1):
    """float64 from the arguments to the images -> (chord lists, ink float64 [B, size, size])"""
    chords = RG.chord_vertices64(commands, args, n=n, groups=groups, fill=fill)
    return chords, torch.stack([RR.image(c["a"].detach(), c["b"].detach(), c["seq"], size, 3.2, fill) for c in chords])


def backward64(commands, chords, ink, dout, fill, n, groups=1):
    """the two restated ops in float64 on float64 chords -> dargs float64"""
    cap = max(len(c["seq"]) for c in chords)
    dsegs = torch.zeros(len(chords), max(cap, 1), 4, dtype=torch.float64)
    for i, c in enumerate(chords):
        a, b = c["a"].detach(), c["b"].detach()
        _, idx = RG.nearest(a, b, ink.shape[-1])
        da, db = RG.chords_bwd(a, b, ink[i], idx, dout[i], fill)
        dsegs[i, :len(da), :2], dsegs[i, :len(da), 2:] = da, db
    counts = torch.tensor([len(c["seq"]) for c in chords], dtype=torch.int32)
    return RG.raster_segments_bwd(commands, dsegs, counts, n=n, groups=groups, fill=fill, as_double=True)


# ---- finite differences -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("size", [8, 16, 33])
def test_restated_gradient_matches_central_differences(size, fill):
    n = 4
    worst, checked = 0.0, 0
    for seed in (1, 2):
        commands, args = outlines(8, seed=100 * size + 10 * seed + int(fill))
        W = torch.rand(8, size, size, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        chords, ink = forward64(commands, args, size, fill, n)
        grad = backward64(commands, chords, ink, W, fill, n)
        for b in range(8):
            def loss(a):
                return float((W[b] * forward64(commands[b:b + 1], a, size, fill, n)[1][0]).sum())
            rows = int((commands[b] != EOS).sum())
            for i in range(rows):
                for col in range(5, 11):
                    hi, lo = args[b:b + 1].clone(), args[b:b + 1].clone()
                    hi[0, i, col] += FD_H
                    lo[0, i, col] -= FD_H
                    fd = (loss(hi) - loss(lo)) / (2 * FD_H)
                    worst = max(worst, abs(fd - grad[b, i, col].item()))
                    checked += 1
        assert bool((grad[..., :5] == 0).all()) and bool((grad[commands == EOS] == 0).all())
    print(f"restated gradient vs central differences size={size} fill={fill}: {checked} coordinates, max err {worst:.3e}")
    assert worst <= FD_ATOL


# ---- the transpose --------------------------------------------------------------------------------------------------------------
def row_cases(L):
    """command rows of length L: a drawing row 0, a drawing row L - 1, an `m` that only supplies a start point, a sub-path of
    one command"""
    if L == 1:
        return [[L_], [C_], [M]]
    pad = [EOS] * L
    return [([C_, L_] + pad)[:L],                                   # row 0 draws, from the constant (0, 0)
            (pad + [M, L_, C_])[-L:],                               # row L - 1 draws
            ([M, M, L_, M, C_, C_] + pad)[:L],                      # the first `m` does nothing, the second and third supply starts
            ([M, C_, M, L_, EOS, L_] + pad)[:L]]                    # sub-paths of one command; an EOS row supplies a start


def case_commands(G, L, seed):
    """[R, L] with R a multiple of G: the row cases, then random rows from the command pool"""
    gen = torch.Generator().manual_seed(seed)
    rows = row_cases(L)
    pool = torch.tensor([0, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6])
    R = -(-(len(rows) + 2 * G) // G) * G
    commands = pool[torch.randint(0, len(pool), (R, L), generator=gen)].float()
    commands[:len(rows)] = torch.tensor(rows, dtype=torch.float32)
    return commands


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("G,L,n", [(1, 9, 2), (3, 7, 5), (2, 1, 4)])
def test_restated_segments_bwd_is_the_transpose_of_the_chord_builder(G, L, n, fill):
    commands = case_commands(G, L, seed=G + L + n)
    R = commands.shape[0]
    gen = torch.Generator().manual_seed(5)
    args = (torch.rand(R, L, 11, generator=gen, dtype=torch.float64) * 256).requires_grad_(True)
    chords = RG.chord_vertices64(commands, args, n=n, groups=G, fill=fill)
    cap = G * (L * (n - 1) + ((L + 1) // 2 if fill else 0))
    dsegs = torch.randn(R // G, max(cap, 1), 4, generator=gen, dtype=torch.float64)
    counts = torch.tensor([len(c["seq"]) for c in chords], dtype=torch.int32)
    assert counts.tolist() == [len(c["seq"]) for c in RR.chord_list(commands, args, n, G, fill)] and int(counts.max()) <= cap
    value = sum((c["a"] * dsegs[i, :len(c["seq"]), :2]).sum() + (c["b"] * dsegs[i, :len(c["seq"]), 2:]).sum()
                for i, c in enumerate(chords))
    want = torch.autograd.grad(value, args)[0] if int(counts.sum()) else torch.zeros_like(args)
    got = RG.raster_segments_bwd(commands, dsegs, counts, n=n, groups=G, fill=fill, as_double=True)
    err = (got - want).abs().max().item()
    print(f"segments_bwd vs autograd through the chord builder G={G} L={L} n={n} fill={fill}: max err {err:.3e}")
    assert err <= 1e-12 * max(1.0, want.abs().max().item())
    assert bool((got[..., :5] == 0).all())
    # a row gets a gradient only if it draws or the row after it does
    draws = (commands == L_) | (commands == C_)
    used = draws.clone()
    used[:, :-1] |= draws[:, 1:]
    assert bool((got[~used] == 0).all()) and bool(got[used].any())
    # the chord builder is the forward restatement with the arguments kept in the graph
    for c, ref in zip(chords, RR.chord_list(commands, args, n, G, fill)):
        assert torch.allclose(c["a"].detach(), ref["a"], rtol=0, atol=1e-10) and torch.allclose(c["b"].detach(), ref["b"], rtol=0, atol=1e-10)


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def rectangle():
    return sequence([(M, 35, 35.5), (L_, 99, 35.5), (L_, 99, 99.5), (L_, 35, 99.5), (L_, 35, 35.5)], 8)


def test_filled_rectangle_under_a_translation_in_x(grad_ops):
    """loss = sum(ink) at size 64 (s = 4): the sixteen left-edge pixels (centres 1 outside x = 35, ink 0.25) give -1/4 each,
    the sixteen right-edge pixels (centres 1 inside x = 99, ink 0.75) +1/4 each; the pixels above the top edge move along it and
    give nothing; what is left is the corner pixel (34, 34) at distance sqrt(1 + 1.5^2) from the corner (35, 35.5):
    -(1 / 4) * (-1 / sqrt(3.25))... with the sign of d ink / d d outside: -1 / (4 sqrt(3.25))"""
    want = -1.0 / (4.0 * np.sqrt(3.25))
    commands, args = rectangle()
    chords, ink = forward64(commands, args.double(), 64, True, 10)
    grad = backward64(commands, chords, ink, torch.ones_like(ink), True, 10)
    live = (ink[0] > 0) & (ink[0] < 1)
    assert int(live[:, 8].sum()) >= 16 and ink[0, 8, 8].item() == pytest.approx(0.5 - np.sqrt(3.25) / 4, abs=1e-12)
    got64 = grad[..., 9].sum().item()
    a = args.clone().requires_grad_(True)
    render.rasterize_with_grad(commands, a, size=64, fill=True).sum().backward()
    got = a.grad[..., 9].sum().item()
    print(f"d sum(ink) / d x of the filled rectangle: float64 {got64:.8f}, through render {got:.8f}, closed form {want:.8f}")
    assert abs(got64 - want) <= 1e-9 and abs(got - want) <= 1e-5
    assert abs(want - (-0.13868)) < 5e-6


def test_the_integer_square_has_an_exactly_zero_gradient_in_fill_mode(grad_ops):
    """every unsaturated pixel of the square (34, 34)-(98, 98) at size 64 sits ON the outline: d == 0 contributes nothing"""
    commands, args = square()
    a = args.clone().requires_grad_(True)
    img = render.rasterize_with_grad(commands, a, size=64, fill=True)
    assert int(((img > 0) & (img < 1)).sum()) == 64
    (img * torch.rand(1, 64, 64, generator=torch.Generator().manual_seed(0))).sum().backward()
    print(f"filled integer square: max |gradient| {a.grad.abs().max().item():.3e}")
    assert bool((a.grad == 0).all())
    # stroked, the same square pulls: the line pixels are at the peak (d == 0) but their neighbours' ink is clamped to 0
    # only from one pixel away on, so a wider stroke leaves live pixels with d > 0
    a = args.clone().requires_grad_(True)
    render.rasterize_with_grad(commands, a, size=64, stroke_width=8.0)[0, :, :16].sum().backward()
    assert bool(a.grad.any())


# ---- wiring -----------------------------------------------------------------------------------------------------------------------
def _icons(seed=3):
    commands, args = outlines(6, seed=seed)
    return commands.view(3, 2, 6), args.float().view(3, 2, 6, 11)


@pytest.mark.parametrize("fill", [False, True])
def test_rasterize_with_grad_has_the_bits_of_rasterize_and_composes_the_two_ops(grad_ops, fill):
    from deepsvg_amd import ops
    commands, args = _icons()
    a = args.clone().requires_grad_(True)
    img = render.rasterize_with_grad(commands, a, size=16, fill=fill, n=4)
    assert img.requires_grad and img.shape == (3, 16, 16)
    assert torch.equal(img.detach().view(torch.int32), render.rasterize(commands, args, size=16, fill=fill, n=4).view(torch.int32))
    rows = render.rasterize_with_grad(commands.reshape(6, 6), args.reshape(6, 6, 11), size=16, fill=fill, n=4)
    assert torch.equal(rows, render.rasterize(commands.reshape(6, 6), args.reshape(6, 6, 11), size=16, fill=fill, n=4))
    dout = torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(1))
    img.backward(dout)
    c, flat = commands.reshape(6, 6), args.reshape(6, 6, 11)
    segs, counts = ops.raster_segments(c, flat, n=4, groups=2, fill=fill)
    out, idx = ops.raster_sweep_nn(segs, counts, size=16, fill=fill)
    want = ops.raster_segments_bwd(c, ops.raster_sweep_bwd(segs, counts, out, idx, dout, fill=fill), counts, n=4, groups=2, fill=fill)
    assert a.grad.shape == args.shape and torch.equal(a.grad, want.view_as(args)) and bool(a.grad.any())
    # integer commands are read as float32; integer arguments have no gradient
    assert torch.equal(render.rasterize_with_grad(commands.long(), args, size=16, fill=fill, n=4), img.detach())
    with pytest.raises(ValueError):
        render.rasterize_with_grad(commands, args.long())
    with pytest.raises(ValueError):
        render.rasterize_with_grad(commands, args[:, :1])
    assert not render.rasterize(commands, a, size=8).requires_grad


def test_image_loss_and_an_empty_image(grad_ops):
    commands, args = _icons()
    commands[1] = EOS                                        # icon 1 draws nothing
    target = torch.rand(3, 16, 16, generator=torch.Generator().manual_seed(2))
    a = args.clone().requires_grad_(True)
    res = render.image_loss(commands, a, target, n=4)
    img = render.rasterize(commands, args, size=16, n=4)
    assert bool((img[1] == 0).all())
    want = (img - target).pow(2).flatten(1).mean(1)
    err = (res["per_icon"] - want).abs().max().item()
    print(f"image_loss per icon vs (rasterize - target)^2: {err:.3e}")
    assert res["per_icon"].shape == (3,) and err <= 1e-7 and res["loss"].item() == pytest.approx(want.mean().item(), abs=1e-7)
    res["loss"].backward()
    assert bool((a.grad[1] == 0).all()) and bool(a.grad[0].any()) and bool(a.grad[2].any())
    with pytest.raises(ValueError):
        render.image_loss(commands, a, target[:2])
    with pytest.raises(ValueError):
        render.image_loss(commands, a, target[:, :8])


def jittered(seed=4, amount=1.5, icons=4):
    """-> commands f32 [icons, 1, 6], target args, start args = target + uniform(-amount, amount) on the rows in use"""
    commands, args = outlines(icons, seed=seed)
    args = args.float()
    jitter = (torch.rand(args.shape, generator=torch.Generator().manual_seed(seed + 1)) * 2 - 1) * amount
    start = torch.where((commands != EOS).unsqueeze(-1), args + jitter, args)
    return commands.view(icons, 1, 6), args.view(icons, 1, 6, 11), start.view(icons, 1, 6, 11)


def test_refine_to_images_lowers_the_loss(grad_ops):
    commands, target_args, start = jittered()
    target = render.rasterize(commands, target_args, size=16, n=4)
    refined, history = render.refine_to_images(commands, start, target, steps=12, lr=0.1, n=4)
    print(f"refine_to_images, 12 steps at 16 x 16: loss {history[0].item():.6f} -> {history[-1].item():.6f}")
    assert history.shape == (12,) and history[-1] < history[0] and refined.dtype == torch.float32 and not refined.requires_grad
    assert torch.equal(refined[..., :5], start[..., :5]) and torch.equal(refined[commands == EOS], start[commands == EOS])
    assert not torch.equal(refined, start)
    assert history[0].item() == pytest.approx(render.image_loss(commands, start, target, n=4)["loss"].item(), abs=1e-7)


def test_refine_to_images_takes_a_list_of_sizes(grad_ops):
    commands, target_args, start = jittered(seed=6)
    targets = [render.rasterize(commands, target_args, size=size, fill=True, n=4) for size in (8, 16)]
    refined, history = render.refine_to_images(commands, start, targets, steps=3, lr=0.1, fill=True, n=4)
    first = sum(render.image_loss(commands, start, t, fill=True, n=4)["loss"].item() for t in targets)
    print(f"refine_to_images on sizes 8 + 16: first loss {history[0].item():.6f} (sum of the two image losses {first:.6f})")
    assert history[0].item() == pytest.approx(first, abs=1e-6) and history.shape == (3,) and not torch.equal(refined, start)
    with pytest.raises(ValueError):
        render.refine_to_images(commands, start, [], steps=1)


# ---- the fp32 spread the GPU bounds rest on -----------------------------------------------------------------------------------------
def spread_case(size, fill):
    """the restated forward on grad_batch() -> (segs, counts, out, idx, dout), all as the ops hand them out"""
    commands, args, G, n = grad_batch()
    segs, counts = RR.raster_segments(commands, args, n=n, groups=G, fill=fill)
    out, idx = RG.raster_sweep_nn(segs, counts, size=size, fill=fill)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(size + int(fill))).clamp(-4, 4)
    return segs, counts, out, idx, dout


def test_fp32_spread_of_the_backward():
    worst, nearest_live = 0.0, float("inf")
    for size, fill in GRAD_CASES:
        segs, counts, out, idx, dout = spread_case(size, fill)
        assert int(counts.min()) > 0 and int(((out > 0) & (out < 1)).sum()) > 0
        d64 = RG.raster_sweep_bwd(segs, counts, out, idx, dout, fill=fill, as_double=True)
        d32 = RG.raster_sweep_bwd(segs, counts, out, idx, dout, fill=fill, dtype=torch.float32)
        spread = (d32.double() - d64).abs().max().item() / dout.abs().max().item()
        live_d = min(RG.smallest_live_distance(*RG._chords_of(segs[i], counts[i]), out[i], idx[i]) for i in range(len(counts)))
        print(f"sweep_bwd fp32 against float64 size={size} fill={fill}: spread {spread:.3e} of max |dout|, smallest live d "
              f"{live_d:.3e}, max |dsegs| {d64.abs().max().item():.3e}")
        worst, nearest_live = max(worst, spread), min(nearest_live, live_d)
    assert nearest_live >= MIN_LIVE_D and worst <= SPREAD


SEG_CASES = [(1, 1), (8, 66), (8, 256)]                    # (G, L) of the GPU test of raster_segments_bwd
SEG_N = [2, 7, 64]


def seg_case(G, L, n, fill, seed=0):
    """-> commands f32 [R, L] (row cases first), dsegs f32 [R / G, cap, 4] standard normal below the counts, counts"""
    commands = case_commands(G, L, seed=seed + G + L + n)
    counts = torch.tensor([len(c["seq"]) for c in RR.chord_list(commands, torch.zeros(*commands.shape, 11), n, G, fill)],
                          dtype=torch.int32)
    cap = G * (L * (n - 1) + ((L + 1) // 2 if fill else 0))
    dsegs = torch.randn(commands.shape[0] // G, max(cap, 1), 4, generator=torch.Generator().manual_seed(seed + 1))
    return commands, dsegs, counts


@pytest.mark.parametrize("fill", [False, True])
def test_fp32_spread_of_segments_bwd(fill):
    worst = 0.0
    for G, L in SEG_CASES:
        for n in SEG_N:
            commands, dsegs, counts = seg_case(G, L, n, fill)
            d64 = RG.raster_segments_bwd(commands, dsegs, counts, n=n, groups=G, fill=fill, as_double=True)
            d32 = RG.raster_segments_bwd(commands, dsegs, counts, n=n, groups=G, fill=fill, dtype=np.float32)
            worst = max(worst, (d32.double() - d64).abs().max().item() / dsegs.abs().max().item())
    print(f"segments_bwd fp32 against float64 fill={fill}: spread {worst:.3e} of max |dsegs|")
    assert worst <= SEG_SPREAD


E2E_SEED, E2E_SIZE, E2E_N = 8, 16, 4
CLAMP_MARGIN, TIE_MARGIN = 1e-3, 1e-3


def e2e_fixture():
    """4 icons of one sequence -> commands f32 [4, 6], args f32 [4, 6, 11]"""
    commands, args = outlines(4, seed=E2E_SEED)
    return commands, args.float()


def fixture_margins(commands, args, size, fill, n):
    """in float64, over all images -> (the smallest distance of an unclamped ink value from 0 and from 1 over all pixels, the
    smallest gap between a live pixel's nearest chord and any chord that shares no vertex with it, the smallest live d)"""
    s = 256.0 / size
    clamp = tie = live_d = float("inf")
    for c in RG.chord_vertices64(commands, args.double(), n=n, fill=fill):
        a, b = c["a"], c["b"]
        d, inside = RR.image(a, b, c["seq"], size, 3.2, fill, return_distance=True)
        raw = torch.where(inside, 0.5 + d / s, 0.5 - d / s) if fill else 0.5 + (1.6 - d) / s
        clamp = min(clamp, raw.abs().min().item(), (raw - 1).abs().min().item())
        live = (raw > 0) & (raw < 1)
        if not bool(live.any()):
            continue
        _, idx = RG.nearest(a, b, size)
        live_d = min(live_d, d[live].min().item())
        for j in range(a.shape[0]):
            mine = live & (idx == j)
            if not bool(mine.any()):
                continue
            apart = ~((a == a[j]).all(1) | (a == b[j]).all(1) | (b == a[j]).all(1) | (b == b[j]).all(1))
            if bool(apart.any()):
                others = torch.stack([RG.distance_to(a, b, torch.full_like(idx, k), size) for k in torch.nonzero(apart).flatten().tolist()])
                tie = min(tie, (others.amin(0) - d)[mine].min().item())
    return clamp, tie, live_d


@pytest.mark.parametrize("fill", [False, True])
def test_fixture_margins(fill):
    clamp, tie, live_d = fixture_margins(*e2e_fixture(), E2E_SIZE, fill, E2E_N)
    print(f"end-to-end fixture fill={fill}: nearest clamp {clamp:.3e} ink, nearest tie {tie:.3e}, smallest live d {live_d:.3e}")
    assert clamp >= CLAMP_MARGIN and tie >= TIE_MARGIN and live_d >= MIN_LIVE_D


def test_binding_declares_the_gradient_entry_points():
    assert lib.ABI_VERSION >= 17
    for name in ("dsvg_raster_sweep_nn", "dsvg_raster_sweep_bwd", "dsvg_raster_segments_bwd"):
        assert name in lib.SIGNATURES
