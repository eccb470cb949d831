"""The gradient of deepsvg_amd.render.draw on CPU: the float64 restatement of tests/raster_layers_grad_ref.py against central
differences (arguments, colours and opacities), against autograd through the chord builder and on a blend chain worked out by
hand; then the host logic of draw_with_grad / picture_loss / refine_to_pictures with the raster ops replaced by the
restatements.  Every test prints the largest error it saw before it asserts.

Inputs (`layered()`): icons of G sequences of `outlines()` (tests/test_render_grad_host.py: one `m` and 3-4 random `l` / `c` with
float arguments rand * 256), modes that cover OUTLINE, FILL, ERASE and the value 7 (an outline), colours in 0.05..0.95 and
opacities in 0.3..0.95 (away from the clamp of the paint: a central difference across it sees the kink).

fp32 spread (test_fp32_spread_of_the_blend_backward): the restated blend backward run in fp32 against float64 on the inputs of
the GPU tests (`BLEND_CASES`), the method of test_fp32_spread_of_the_backward:
  BLEND_SPREAD = 8.5e-8 (dcov, of max |dout|; dcov itself reaches 3.7): measured 7.98e-8, at size 100 with 8 layers.
  PAINT_SPREAD = 2.0e-9 (dpaint, of max |dout| times the pixels of an image; dpaint reaches 33): the fp32 run sums the pixels
  ONE AFTER THE OTHER in pixel order (np.cumsum), the longest chain an fp32 sum over the pixels can have - the kernel's tree
  per 64 pixels and torch's pairwise sum are both shorter; measured 1.87e-9, at size 33.
The GPU tests allow the kernel 4 x these.  The chord and the segment backward have the formulas of the one-channel gradient
and reuse SPREAD and SEG_SPREAD of tests/test_render_grad_host.py.  SPREAD was measured with every live pixel at least
MIN_LIVE_D = 1e-2 from its chord, and the cases of SWEEP_CASES (seeds chosen for it) carry it as it is.  Two cases cannot meet
that margin - 16 sequences at size 100 have thousands of live pixels, the `long` batch has integer arguments - and carry
`sweep_spread(live_d)` = SPREAD * MIN_LIVE_D / live_d instead: a pixel's term is dcov / (s d) times q, and q = p - a - t (b - a)
is formed in fp32 from coordinates of up to 256 with an absolute error that does not depend on d, so the error of the
direction q / d, and with it the spread, grows as 1 / d (the docstring of tests/test_render_grad_host.py says the same of
SPREAD).  test_fp32_spread_of_the_chord_backward measures it on every case: 5.78e-5 at `g8_s100` (smallest live d 1.14e-3, bound
1.05e-4) and 4.54e-6 at `long` (7.76e-4, bound 1.55e-4).

The end-to-end fixture of the GPU tests (`e2e_layers()`, margins stated by test_layered_fixture_margins with fixture_margins
of tests/test_render_grad_host.py, held in EVERY layer): in float64 no coverage lies within 1e-3 of a clamp, no live pixel has a
chord of its layer that shares no vertex with its nearest one within 1e-3 of it, and no live pixel is closer than 1e-2 to its
chord - so the float64 restatement from the arguments, with its own coverage and its own arg-min, picks the pixels and chords
the fp32 kernels pick.  No pixel is excluded anywhere."""
import numpy as np
import pytest
import torch

from deepsvg_amd import lib, render
from tests import raster_grad_ref as RG
from tests import raster_layers_grad_ref as LG
from tests import raster_layers_ref as LR
from tests import raster_ref as RR
from tests.test_draw_host import BLUE, RED, ring, two_square_pixels, two_squares
from tests.test_render_grad_host import (CLAMP_MARGIN, FD_ATOL, FD_H, MIN_LIVE_D, SPREAD, TIE_MARGIN, case_commands,
                                         fixture_margins, outlines)
from tests.test_render_host import EOS, L_, C_

BLEND_SPREAD, PAINT_SPREAD = 8.5e-8, 2.0e-9


@pytest.fixture
def layer_ops(emulated_ops):
    saved = LG.install()
    yield
    LG.restore(saved)


def layered(N, G, seed, modes=None):
    """N icons of G sequences of outlines() -> commands f32 [N * G, 6], args float64 [N * G, 6, 11], modes int32 [N, G] (given, or
    random from 0, 1, 2, 7), paint float64 [N, G, 4] (colours 0.05..0.95, opacities 0.3..0.95), background (three numbers)"""
    commands, args = outlines(N * G, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    if modes is None:
        modes = torch.tensor([0, 1, 2, 7])[torch.randint(0, 4, (N, G), generator=gen)]
    modes = torch.as_tensor(modes, dtype=torch.int32).view(N, G)
    paint = torch.rand(N, G, 4, generator=gen, dtype=torch.float64)
    paint[..., :3] = 0.05 + 0.9 * paint[..., :3]
    paint[..., 3] = 0.3 + 0.65 * paint[..., 3]
    return commands, args, modes, paint, (0.05 + 0.9 * torch.rand(3, generator=gen, dtype=torch.float64)).tolist()


# ---- finite differences -------------------------------------------------------------------------------------------------------
FD_RULES = [(None, False), (None, True), ("fill", False), ("fill", True), ("stroke", False)]          # (compound, evenodd)


@pytest.mark.parametrize("compound,evenodd", FD_RULES)
@pytest.mark.parametrize("size", [16, 33])
def test_restated_gradient_matches_central_differences(size, compound, evenodd):
    N, G, n = 2, 3, 4
    commands, args, modes, paint, background = layered(N, G, seed=10 * size + len(FD_RULES) * int(evenodd) + (len(compound) if compound else 0),
                                                       modes=[[1, 2, 0], [7, 1, 2]])
    m = None if compound else modes.tolist()
    kw = dict(background=background, size=size, evenodd=evenodd, compound=compound, n=n, groups=G)
    W = torch.rand(N, 3, size, size, generator=torch.Generator().manual_seed(size), dtype=torch.float64)
    out, state = LG.picture64(commands, args, m, paint, **kw)
    dargs, dpaint = LG.picture_backward64(commands, state, paint, W, background=background, compound=compound, n=n, groups=G)

    def loss(a, p):
        return float((W * LG.picture64(commands, a, m, p, **kw)[0]).sum())

    worst, checked = 0.0, 0
    for row in range(N * G):
        for i in range(int((commands[row] != EOS).sum())):
            for col in range(5, 11):
                hi, lo = args.clone(), args.clone()
                hi[row, i, col] += FD_H
                lo[row, i, col] -= FD_H
                fd = (loss(hi, paint) - loss(lo, paint)) / (2 * FD_H)
                worst = max(worst, abs(fd - dargs[row, i, col].item()))
                checked += 1
    worst_paint = 0.0
    for i in range(N):
        for g in range(G):
            for k in range(4):
                hi, lo = paint.clone(), paint.clone()
                hi[i, g, k] += FD_H
                lo[i, g, k] -= FD_H
                fd = (loss(args, hi) - loss(args, lo)) / (2 * FD_H)
                worst_paint = max(worst_paint, abs(fd - dpaint[i, g, k].item()))
    print(f"restated layered gradient vs central differences size={size} compound={compound} evenodd={evenodd}: {checked} "
          f"argument coordinates, max err {worst:.3e}; colours and opacities max err {worst_paint:.3e}")
    assert bool((dargs[..., :5] == 0).all()) and bool((dargs[commands == EOS] == 0).all()) and bool(dargs.any())
    if compound:
        assert bool((dpaint[:, 1:] == 0).all()) and bool(dpaint[:, 0].all()), "a compound picture has the paint of group 0"
    else:
        erase = modes == 2
        # (an ERASE layer has no colour; its opacity moves the picture only where it lies over paint)
        assert bool((dpaint[..., :3][erase] == 0).all()) and bool(dpaint[~erase].all())
    assert worst <= FD_ATOL and worst_paint <= FD_ATOL * size * size / 256


# ---- the transpose --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,L,n", [(1, 9, 2), (3, 7, 5), (4, 6, 4)])
def test_restated_segments_layers_bwd_is_the_transpose_of_the_chord_builder(G, L, n):
    commands = case_commands(G, L, seed=G + L + n)
    R = commands.shape[0]
    gen = torch.Generator().manual_seed(6)
    modes = torch.tensor([0, 1, 2, 7])[torch.randint(0, 4, (R // G, G), generator=gen)]
    modes[0, 0], modes[1, 0] = 1, 0                         # (the row cases are drawn closed and open)
    args = (torch.rand(R, L, 11, generator=gen, dtype=torch.float64) * 256).requires_grad_(True)
    layers = LG.layer_vertices64(commands, args, modes.tolist(), n=n, groups=G)
    cap = G * (L * (n - 1) + (L + 1) // 2)
    dsegs = torch.randn(R // G, cap, 4, generator=gen, dtype=torch.float64)
    counts = torch.tensor([sum(a.shape[0] for a, _, _ in ly) for ly in layers], dtype=torch.int32)
    want_counts = [sum(ly["a"].shape[0] for ly in icon) for icon in LR.group_chords(commands, args.detach(), modes.tolist(), n, G)]
    assert counts.tolist() == want_counts and int(counts.max()) <= cap
    value = 0.0
    for i, ly in enumerate(layers):
        a, b = torch.cat([t[0] for t in ly]), torch.cat([t[1] for t in ly])
        value = value + (a * dsegs[i, :a.shape[0], :2]).sum() + (b * dsegs[i, :a.shape[0], 2:]).sum()
    want = torch.autograd.grad(value, args)[0]
    got = LG.raster_segments_layers_bwd(commands, dsegs, counts, modes, n=n, groups=G, as_double=True)
    err = (got - want).abs().max().item()
    print(f"segments_layers_bwd vs autograd through the chord builder G={G} L={L} n={n}: max err {err:.3e}")
    assert err <= 1e-12 * max(1.0, want.abs().max().item()) and bool(want.any())
    assert bool((got[..., :5] == 0).all())
    closed = ((modes == 1) | (modes == 2)).any().item() and not ((modes == 1) | (modes == 2)).all().item()
    assert closed, "the modes of this case are not mixed"
    # with one mode for every group it is raster_segments_bwd
    for mode, fill in ((0, False), (2, True)):
        uniform = torch.full_like(modes, mode)
        k = torch.tensor([len(c["seq"]) for c in RR.chord_list(commands, args.detach(), n, G, fill)], dtype=torch.int32)
        one = LG.raster_segments_layers_bwd(commands, dsegs, k, uniform, n=n, groups=G, as_double=True)
        assert torch.equal(one, RG.raster_segments_bwd(commands, dsegs, k, n=n, groups=G, fill=fill, as_double=True))


# ---- the blend chain by hand ---------------------------------------------------------------------------------------------------
def _two_square_forward(colors, opacity, modes=(1, 1), size=64):
    commands, args = two_squares()
    c, a = commands.reshape(2, -1), args.reshape(2, -1, 11)
    m = torch.tensor([list(modes)], dtype=torch.int32)
    paint = torch.cat([torch.as_tensor(colors, dtype=torch.float32).view(1, 2, 3),
                       torch.as_tensor(opacity, dtype=torch.float32).view(1, 2, 1)], -1)
    segs, counts, first = LR.raster_segments_layers(c, a, m, n=10, groups=2)
    out, cov, idx = LG.raster_sweep_layers_nn(segs, counts, first, m, paint, size=size)
    return (segs, counts, first, m, paint), out, cov, idx


def test_two_layers_at_half_opacity_follow_the_chain_by_hand():
    """RED then BLUE at opacity 0.5 on white, dout = 1 in every channel at a pixel of the first square only and at one of the
    overlap.  Overlap: C_1 = (1, .5, .5); sum_c (BLUE_c - C_1,c) = -1 -> d alpha_2 = -1; sum_c (RED_c - 1) = -2, T_1 = 0.5 -> d alpha_1
    = -1; d colour_2 = alpha_2 = 0.5, d colour_1 = T_1 alpha_1 = 0.25.  First square only (cov_2 = 0, T_1 = 1): d alpha_1 = -2, d alpha_2
    = -1 (with cov_2 = 0 it moves no opacity), d colour_1 = 0.5.  dcov = d alpha * 0.5, d opacity = d alpha * cov"""
    tables, out, cov, idx = _two_square_forward([RED, BLUE], [0.5, 0.5])
    first, both, _, _ = two_square_pixels()
    assert out[0, :, both[0], both[1]].tolist() == [0.5, 0.25, 0.75] and cov[0, :, both[0], both[1]].tolist() == [1.0, 1.0]
    assert cov[0, :, first[0], first[1]].tolist() == [1.0, 0.0]
    dout = torch.zeros(1, 3, 64, 64)
    dout[0, :, both[0], both[1]] = 1.0
    dout[0, :, first[0], first[1]] = 1.0
    segs, counts, layer_first, modes, paint = tables
    for dtype in (torch.float64, torch.float32):
        dcov, dpaint = LG.raster_blend_bwd(cov, counts, layer_first, modes, paint, dout, segs.shape[1], dtype=dtype)
        assert dcov[0, :, both[0], both[1]].tolist() == [-0.5, -0.5] and dcov[0, :, first[0], first[1]].tolist() == [-1.0, -0.5]
        assert int((dcov != 0).sum()) == 4
        assert dpaint[0].tolist() == [[0.75, 0.75, 0.75, -3.0], [0.5, 0.5, 0.5, -1.0]]


def test_erase_skipped_and_clamped_paint_get_exact_zeros():
    commands, args, modes, paint, background = layered(3, 4, seed=3, modes=[[1, 2, 0, 1], [2, 7, 1, 0], [1, 1, 0, 2]])
    commands[2] = EOS                                        # icon 0: an empty group between two drawn ones
    commands[4:8] = EOS                                      # icon 1 draws nothing
    paint[0, 3, 0], paint[0, 0, 1], paint[0, 0, 2], paint[0, 0, 3] = 1.5, float("nan"), 1.0, 1.0
    paint[2, 0, 3], paint[2, 1, 3], paint[2, 2, 3] = 1.75, -0.25, float("nan")
    a = args.float()
    segs, counts, first = LR.raster_segments_layers(commands, a, modes, n=4, groups=4)
    p32 = paint.float()
    out, cov, idx = LG.raster_sweep_layers_nn(segs, counts, first, modes, p32, background=background, size=16)
    assert int(counts[1]) == 0 and bool((cov[1] == 0).all()) and bool((idx[1] == -1).all()) and bool((cov[0, 2] == 0).all())
    assert torch.equal(idx == -1, ~((cov > 0) & (cov < 1)))
    dout = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    dcov, dpaint = LG.raster_blend_bwd(cov, counts, first, modes, p32, dout, segs.shape[1], background=background)
    assert bool((dcov[1] == 0).all()) and bool((dpaint[1] == 0).all()), "an icon without chords"
    assert bool((dcov[0, 2] == 0).all()) and bool((dpaint[0, 2] == 0).all()), "a skipped layer"
    assert bool((dpaint[0, 1, :3] == 0).all()) and dpaint[0, 1, 3] != 0, "an ERASE layer has no colour, but an opacity"
    assert dpaint[0, 3, 0] == 0 and dpaint[0, 0, 1] == 0 and bool((dpaint[2, :3, 3] == 0).all()), "clamped or NaN paint"
    assert dpaint[0, 0, 2] != 0 and dpaint[0, 0, 3] != 0, "a value ON the clamp passes the gradient"
    assert dpaint[0, 0, 0] != 0 and dpaint[0, 3, 1] != 0 and bool(dpaint[2, 0, :3].all()), "the neighbours of a clamped value"
    assert bool(torch.isfinite(dcov).all()) and bool(torch.isfinite(dpaint).all())


def test_an_opaque_fill_hides_what_lies_below_without_a_division():
    """opacity 1 inside the second square: 1 - alpha = 0 there, T = 0 for the first layer, and nothing is NaN"""
    tables, out, cov, idx = _two_square_forward([RED, BLUE], [1.0, 1.0])
    segs, counts, layer_first, modes, paint = tables
    dout = torch.tensor([1.0, 0.5, 0.25]).view(1, 3, 1, 1).expand(1, 3, 64, 64).contiguous()
    dcov, dpaint = LG.raster_blend_bwd(cov, counts, layer_first, modes, paint, dout, segs.shape[1])
    _, both, second, _ = two_square_pixels()
    assert bool(torch.isfinite(dcov).all()) and bool(torch.isfinite(dpaint).all())
    assert dcov[0, 0, both[0], both[1]] == 0 and dcov[0, 1, both[0], both[1]] != 0 and dcov[0, 1, second[0], second[1]] != 0


# ---- wiring -----------------------------------------------------------------------------------------------------------------------
def _icons(seed=3, N=3, G=2):
    commands, args, modes, paint, background = layered(N, G, seed=seed, modes=[[1, 2], [0, 1], [7, 2]])
    return commands.view(N, G, 6), args.float().view(N, G, 6, 11), modes, paint.float(), background


@pytest.mark.parametrize("compound", [False, True])
def test_draw_with_grad_has_the_bits_of_draw_and_composes_the_ops(layer_ops, compound):
    from deepsvg_amd import ops
    commands, args, modes, paint, background = _icons()
    kw = dict(compound=True, fill=True, fill_rule="evenodd") if compound else dict(filling=modes)
    kw.update(background=background, size=16, n=4)
    a = args.clone().requires_grad_(True)
    colors, opacity = paint[0, :, :3].clone().requires_grad_(True), paint[..., 3].clone().requires_grad_(True)
    img = render.draw_with_grad(commands, a, colors=colors, opacity=opacity, **kw)
    assert img.requires_grad and img.shape == (3, 3, 16, 16)
    want = render.draw(commands, args, colors=colors.detach(), opacity=opacity.detach(), **kw)
    assert torch.equal(img.detach().view(torch.int32), want.view(torch.int32))
    dout = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    img.backward(dout)
    c, flat = commands.reshape(6, 6), args.reshape(6, 6, 11)
    p = torch.cat([colors.detach().expand(3, 2, 3), opacity.detach().unsqueeze(-1)], -1).contiguous()
    mode = "fill" if compound else None
    m = None if compound else modes
    out, saved = ops.draw_fwd_nn(c, flat, m, p, background=background, size=16, evenodd=compound, compound=mode, n=4, groups=2)
    dargs, dpaint = ops.draw_bwd(c, m, p, saved, dout, background=background, compound=mode, n=4, groups=2)
    assert torch.equal(out, want)
    assert a.grad.shape == args.shape and torch.equal(a.grad, dargs.view_as(args)) and bool(a.grad.any())
    assert colors.grad.shape == (2, 3) and torch.allclose(colors.grad, dpaint[..., :3].sum(0), rtol=1e-6, atol=1e-7)
    assert opacity.grad.shape == (3, 2) and torch.equal(opacity.grad, dpaint[..., 3]) and bool(opacity.grad[:, 0].all())
    # a [N, S] batch is G = 1; integer commands are read as float32; integer arguments have no gradient
    rows = render.draw_with_grad(commands[:, 0], args[:, 0], fill=True, size=16, n=4)
    assert torch.equal(rows, render.draw(commands[:, 0], args[:, 0], fill=True, size=16, n=4))
    assert torch.equal(render.draw_with_grad(commands.long(), args, colors=colors, opacity=opacity, **kw), img)
    with pytest.raises(ValueError, match="float32 args"):
        render.draw_with_grad(commands, args.long(), **kw)
    with pytest.raises(ValueError):
        render.draw_with_grad(commands, args[:, :1], **kw)
    for bad in (dict(colors=torch.zeros(3, 3)), dict(opacity=torch.ones(3)), dict(fill_rule="winding"), dict(opacity=1.5),
                dict(background=(1.0, 1.0)), dict(filling=torch.tensor([[1.0, 2.0]] * 3), compound=False)):
        with pytest.raises(ValueError, match="draw_with_grad"):
            render.draw_with_grad(commands, args, **{**kw, **bad})
    assert not render.draw(commands, a, **kw).requires_grad


def test_picture_loss_and_an_empty_icon(layer_ops):
    commands, args, modes, paint, background = _icons()
    commands[1] = EOS                                        # icon 1 draws nothing
    target = torch.rand(3, 3, 16, 16, generator=torch.Generator().manual_seed(2))
    a = args.clone().requires_grad_(True)
    kw = dict(filling=modes, colors=paint[..., :3], opacity=paint[..., 3], background=background, n=4)
    res = render.picture_loss(commands, a, target, **kw)
    img = render.draw(commands, args, size=16, **kw)
    assert torch.equal(img[1], torch.tensor(background).view(3, 1, 1).expand(3, 16, 16).float())
    want = (img - target).pow(2).flatten(1).mean(1)
    err = (res["per_icon"] - want).abs().max().item()
    print(f"picture_loss per icon vs (draw - target)^2: {err:.3e}")
    assert res["per_icon"].shape == (3,) and err <= 1e-7 and res["loss"].item() == pytest.approx(want.mean().item(), abs=1e-7)
    res["loss"].backward()
    assert bool((a.grad[1] == 0).all()) and bool(a.grad[0].any()) and bool(a.grad[2].any())
    with pytest.raises(ValueError):
        render.picture_loss(commands, a, target[:2], **kw)
    with pytest.raises(ValueError):
        render.picture_loss(commands, a, target[:, 0], **kw)


def shifted_ring(shift=1.5, offset=0.37):
    """the ring of tests/test_draw_host.py with its vertices moved off the pixel centres by `offset` -> commands [1, 2, 8], the
    target's args, the start's args (the inner square moved by `shift` in x and y)"""
    commands, args = ring()
    target = args.clone()
    target[..., 9:11] = torch.where(commands.unsqueeze(-1) != EOS, args[..., 9:11] + offset, args[..., 9:11])
    start = target.clone()
    start[0, 1, :, 9:11] = torch.where(commands[0, 1].unsqueeze(-1) != EOS, target[0, 1, :, 9:11] + shift, target[0, 1, :, 9:11])
    return commands, target, start


def test_refine_to_pictures_moves_the_hole_of_a_ring(layer_ops):
    commands, target_args, start = shifted_ring()
    filling = torch.tensor([[1, 2]])
    target = render.draw(commands, target_args, filling=filling, size=16)
    refined, history = render.refine_to_pictures(commands, start, target, steps=12, lr=0.1, filling=filling)
    before = (start[0, 1, :5, 9:11] - target_args[0, 1, :5, 9:11]).abs().mean().item()
    after = (refined[0, 1, :5, 9:11] - target_args[0, 1, :5, 9:11]).abs().mean().item()
    print(f"refine_to_pictures, 12 steps at 16 x 16: loss {history[0].item():.6f} -> {history[-1].item():.6f}; the inner vertices are "
          f"{before:.3f} -> {after:.3f} from the target's")
    assert history.shape == (12,) and history[-1] < history[0] and after < before
    assert refined.dtype == torch.float32 and not refined.requires_grad
    assert torch.equal(refined[..., :5], start[..., :5]) and torch.equal(refined[commands == EOS], start[commands == EOS])
    assert history[0].item() == pytest.approx(render.picture_loss(commands, start, target, filling=filling)["loss"].item(), abs=1e-7)
    # a list of sizes
    targets = [render.draw(commands, target_args, filling=filling, size=size) for size in (8, 16)]
    _, history = render.refine_to_pictures(commands, start, targets, steps=2, lr=0.1, filling=filling)
    first = sum(render.picture_loss(commands, start, t, filling=filling)["loss"].item() for t in targets)
    assert history[0].item() == pytest.approx(first, abs=1e-6)
    with pytest.raises(ValueError):
        render.refine_to_pictures(commands, start, [], steps=1)


# ---- the fp32 spread the GPU bounds rest on -----------------------------------------------------------------------------------------
BLEND_CASES = {          # name -> (N, G, size, n, seed, modes or None, compound)
    "g1_s8": (2, 1, 8, 4, 41, [[1], [0]], None),
    "g3_s33": (4, 3, 33, 4, 78, [[1, 2, 0], [7, 1, 1], [2, 0, 1], [1, 1, 2]], None),
    "g8_s100": (2, 8, 100, 4, 43, None, None),
    "g3_s100": (1, 3, 100, 4, 118, [[1, 2, 0]], None),
    "g8_s16": (2, 8, 16, 4, 47, None, None),
    "g3_s33_compound": (4, 3, 33, 4, 78, None, "fill"),
    "gaps_s33": (3, 3, 33, 4, 44, [[1, 2, 7], [0, 1, 2], [2, 1, 0]], None),
}


# the cases whose smallest live distance (float64, restated forward) is >= MIN_LIVE_D, the condition SPREAD was measured
# under: the seeds were chosen for it, and the GPU test of the chord backward asserts it on the kernel's own forward.  At
# size 100 with 16 sequences no seed has it (thousands of live pixels, each below 1e-2 with probability about 1 / 200), and
# the integer arguments of `long` do not either: those two carry sweep_spread(live_d)
SWEEP_CASES = ["g1_s8", "g3_s33", "g3_s100", "g8_s16", "g3_s33_compound", "gaps_s33"]


def sweep_spread(live_d):
    """the fp32 spread of the chord backward, of max |dcov|, when the smallest live distance is live_d (module docstring)"""
    return SPREAD * max(1.0, MIN_LIVE_D / live_d)


LONG_MODES = [[1, 0, 2, 7, 1, 2, 0, 1], [0, 1, 1, 2, 7, 1, 2, 0]]


def blend_case(name):
    """-> (commands f32 [N * G, L], args f32, modes int32 [N, G] or None, paint f32 [N, G, 4], background, dict(size, n, groups,
    compound, evenodd)).  `gaps`: icon 0 has an empty group between two drawn ones, icon 1 draws nothing.  `long`: the batch
    of that name of tests/test_render_gpu.py (2 icons of 8 x 66 tokens with integer arguments, n = 10: more chords in an
    image than one chord tile of the sweep, layers that end inside a tile and layers that run across two; groups 3 and 7 of
    icon 0 and 3, 6, 7 of icon 1 are empty) at size 33"""
    if name == "long":
        from tests.test_metrics_gpu import _random_sequences
        commands, args = _random_sequences(2, 8, 66, seed=21)
        _, _, modes, paint, background = layered(2, 8, seed=21, modes=LONG_MODES)
        return (commands.reshape(16, 66).float(), args.reshape(16, 66, 11).float(), modes, paint.float(), background,
                dict(size=33, n=10, groups=8, compound=None, evenodd=False))
    N, G, size, n, seed, modes, compound = BLEND_CASES[name]
    commands, args, modes, paint, background = layered(N, G, seed=seed, modes=modes)
    if name.startswith("gaps"):
        commands[1] = EOS
        commands[G:2 * G] = EOS
    return (commands, args.float(), None if compound else modes, paint.float(), background,
            dict(size=size, n=n, groups=G, compound=compound, evenodd=bool(compound)))


def blend_dout(name, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(len(name))).clamp(-4, 4)


def one_after_the_other(terms):
    """[k, pixels] fp32 -> [k]: the sum taken one pixel after the other, in fp32"""
    return torch.from_numpy(np.cumsum(terms.numpy(), axis=-1, dtype=np.float32)[..., -1])


def restated_forward(name):
    """the restated forward on blend_case(name) -> (tables (segs, counts, first, modes, paint), background, kw, cov, idx, dout)"""
    commands, args, modes, paint, background, kw = blend_case(name)
    G, compound = kw["groups"], kw["compound"]
    if compound:
        segs, counts = RR.raster_segments(commands, args, n=kw["n"], groups=G, fill=True)
        first = None
    else:
        segs, counts, first = LR.raster_segments_layers(commands, args, modes, n=kw["n"], groups=G)
    out, cov, idx = LG.raster_sweep_layers_nn(segs, counts, first, modes, paint, background=background, size=kw["size"],
                                              evenodd=kw["evenodd"], compound=compound)
    return (segs, counts, first, modes, paint), background, kw, cov, idx, blend_dout(name, out.shape)


def smallest_live_distance(segs, counts, cov, idx):
    """over all images and layers: the smallest float64 distance of a pixel that carries a gradient to the chord it names"""
    best = float("inf")
    for i in range(segs.shape[0]):
        a, b = LG._records64(segs[i], counts[i])
        best = min([best] + [RG.smallest_live_distance(a, b, cov[i, g], idx[i, g]) for g in range(cov.shape[1])])
    return best


def test_fp32_spread_of_the_chord_backward():
    for name in [*BLEND_CASES, "long"]:
        (segs, counts, first, modes, paint), background, kw, cov, idx, dout = restated_forward(name)
        compound = kw["compound"]
        dcov, _ = LG.raster_blend_bwd(cov, counts, first, modes, paint, dout, segs.shape[1], background=background, compound=compound)
        d64 = LG.raster_sweep_layers_bwd(segs, counts, first, modes, cov, idx, dcov, compound=compound, as_double=True)
        d32 = LG.raster_sweep_layers_bwd(segs, counts, first, modes, cov, idx, dcov, compound=compound, dtype=torch.float32)
        spread = (d32.double() - d64).abs().max().item() / dcov.abs().max().item()
        live_d = smallest_live_distance(segs, counts, cov, idx)
        print(f"sweep_layers_bwd fp32 against float64 `{name}`: spread {spread:.3e} of max |dcov|, smallest live d {live_d:.3e}, bound "
              f"{sweep_spread(live_d):.3e}, max |dsegs| {d64.abs().max().item():.3e}")
        assert live_d > 0 and bool(d64.any()) and spread <= sweep_spread(live_d)
        assert (live_d >= MIN_LIVE_D) == (name in SWEEP_CASES), "SWEEP_CASES are the cases that hold the margin SPREAD assumes"


def test_fp32_spread_of_the_blend_backward():
    worst_cov = worst_paint = 0.0
    for name in [*BLEND_CASES, "long"]:
        (segs, counts, first, modes, paint), background, kw, cov, idx, dout = restated_forward(name)
        compound = kw["compound"]
        want_cov, want_paint = LG.raster_blend_bwd(cov, counts, first, modes, paint, dout, segs.shape[1], background=background,
                                                   compound=compound, as_double=True)
        got_cov, got_paint = LG.raster_blend_bwd(cov, counts, first, modes, paint, dout, segs.shape[1], background=background,
                                                 compound=compound, dtype=torch.float32, sum_pixels=one_after_the_other)
        scale = dout.abs().max().item()
        s_cov = (got_cov.double() - want_cov).abs().max().item() / scale
        s_paint = (got_paint.double() - want_paint).abs().max().item() / (scale * kw["size"] ** 2)
        print(f"blend_bwd fp32 against float64 `{name}`: dcov spread {s_cov:.3e} of max |dout|, dpaint spread {s_paint:.3e} of max "
              f"|dout| x pixels; max |dcov| {want_cov.abs().max().item():.3e}, max |dpaint| {want_paint.abs().max().item():.3e}")
        assert bool(want_cov.any()) and bool(want_paint.any())
        worst_cov, worst_paint = max(worst_cov, s_cov), max(worst_paint, s_paint)
    assert worst_cov <= BLEND_SPREAD and worst_paint <= PAINT_SPREAD


# ---- the end-to-end fixture -----------------------------------------------------------------------------------------------------------
E2E_SEED, E2E_SIZE, E2E_N, E2E_G = 0, 16, 4, 3
E2E_MODES = [[1, 2, 0], [0, 1, 2]]


def e2e_layers():
    """2 icons of 3 layers, every mode in both -> commands f32 [6, 6], args f32 [6, 6, 11], modes int32 [2, 3], paint f32
    [2, 3, 4], background"""
    commands, args, modes, paint, background = layered(2, E2E_G, seed=E2E_SEED, modes=E2E_MODES)
    return commands, args.float(), modes, paint.float(), background


def layered_margins(commands, args, modes):
    """fixture_margins over the layers of each kind: a layer is one sequence drawn with its own chords"""
    closed = torch.tensor([LR.norm_mode(m) != LR.OUTLINE for m in modes.flatten().tolist()])
    parts = [fixture_margins(commands[sel], args[sel], E2E_SIZE, fill, E2E_N) for sel, fill in ((closed, True), (~closed, False))]
    return tuple(min(p[k] for p in parts) for k in range(3))


def test_layered_fixture_margins():
    commands, args, modes, paint, background = e2e_layers()
    clamp, tie, live_d = layered_margins(commands, args, modes)
    print(f"layered end-to-end fixture: nearest clamp {clamp:.3e} of coverage, nearest tie {tie:.3e}, smallest live d {live_d:.3e}")
    assert clamp >= CLAMP_MARGIN and tie >= TIE_MARGIN and live_d >= MIN_LIVE_D
    assert sorted(set(modes.flatten().tolist())) == [0, 1, 2]


def test_binding_declares_the_layered_gradient_entry_points():
    assert lib.ABI_VERSION == 19
    for name, n_args in (("dsvg_raster_sweep_layers_nn", 16), ("dsvg_raster_blend_bwd", 15), ("dsvg_raster_sweep_layers_bwd", 15),
                         ("dsvg_raster_segments_layers_bwd", 10)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n_args
    for name in ("draw_with_grad", "picture_loss", "refine_to_pictures"):
        assert name in render.__all__
