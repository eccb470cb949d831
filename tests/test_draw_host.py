"""deepsvg_amd.render.draw on CPU: the float64 restatement of a layered image (tests/raster_layers_ref.py) on cases whose
pictures are known in closed form, and the host logic of `draw` with the three layered raster ops replaced by the
restatement.

Tolerance of a layered image against the restatement, per pixel and channel: K * ink_atol(size) + K * 2**-22 with K the
number of layers of the icon that have chords.  A blend canvas + alpha (p - canvas) is 1-Lipschitz in the canvas (0 <= alpha
<= 1) and |p - canvas| <= 1, so a layer adds at most the error of its own coverage - ink_atol of tests/test_render_host.py, the
factor 2 for a pixel whose inside test is decided by rounding included - plus the rounding of the blend: alpha = opacity *
cov, p - canvas, the product and the sum, four roundings of values <= 1, 4 * 2**-24 = 2**-22 (the kernel's fmaf has three).
The share of the fp32 arithmetic, checked here (test_fp32_formulas_stay_within_their_share_of_the_bound): K * (FP32_ATOL / s +
2**-22) with FP32_ATOL of tests/test_render_host.py - random icons of tests/test_metrics_gpu.py::_random_sequences with random
modes, colours and opacities, sizes 8, 64 and 100, n = 2 and 10, both fill rules, layered and compound; largest seen here:
1.08e-5 / s (4.2e-6 in ink, compound stroke at size 100) against a coverage share of 4.4e-5 / s per layer."""
import pytest
import torch

from deepsvg_amd import lib, render
from tests import raster_layers_ref as LR
from tests.test_render_host import EOS, FP32_ATOL, ink_atol, raster_ops, square, square_masks  # noqa: F401

RED, BLUE = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)


def layered_atol(size, layers):
    return layers * ink_atol(size) + layers * 2.0 ** -22


@pytest.fixture
def draw_ops(raster_ops):
    saved = LR.install()
    yield
    LR.restore(saved)


def icon(*groups):
    """sequences (commands [1, S], args [1, S, 11]) -> commands [1, G, S], args [1, G, S, 11]"""
    return torch.stack([c[0] for c, _ in groups])[None], torch.stack([a[0] for _, a in groups])[None]


def ring():
    return icon(square(34, 98), square(50, 82))


def ring_masks():
    """pixel classes of the ring at size 64: strictly inside the inner square, strictly between the squares, on either
    outline, strictly outside"""
    inner_in, inner_edge, _ = square_masks(lo=12, hi=20)
    outer_in, outer_edge, outside = square_masks()
    return inner_in, outer_in & ~inner_in & ~inner_edge, inner_edge | outer_edge, outside


def _check_ring(img):
    hole, band, edge, outside = ring_masks()
    assert img.shape == (3, 64, 64) and img.dtype == torch.float32
    assert int(hole.sum()) == 49 and int(edge.sum()) == 64 + 32
    for ch in img:
        assert bool((ch[hole] == 1.0).all()), "the erase path did not open the hole"
        assert bool((ch[band] == 0.0).all()) and bool((ch[outside] == 1.0).all())
        assert (ch[edge] - 0.5).abs().max().item() <= layered_atol(64, 2)


def test_ring_fill_then_erase(draw_ops):
    commands, args = ring()
    _check_ring(render.draw(commands, args, filling=torch.tensor([[1, 2]]), size=64)[0])
    _check_ring(render.draw(commands, args, filling=torch.tensor([[[1], [2]]]), size=64)[0])      # [N, G, 1], as the data sets


def test_compound_even_odd_is_the_ring_and_non_zero_the_disc(draw_ops):
    commands, args = ring()
    layered = render.draw(commands, args, filling=torch.tensor([[1, 2]]), size=64)
    evenodd = render.draw(commands, args, compound=True, fill=True, fill_rule="evenodd", size=64)
    assert torch.equal(evenodd, layered)
    disc = render.draw(commands, args, compound=True, fill=True, fill_rule="nonzero", size=64)[0]
    hole, band, _, outside = ring_masks()
    assert bool((disc[:, hole] == 0.0).all()) and bool((disc[:, band] == 0.0).all()) and bool((disc[:, outside] == 1.0).all())
    # a compound outline is the stroke image of all chords
    # (the emulation rounds 1 - cov once from float64, the device twice: tests/test_draw_gpu.py pins the bits)
    stroke = render.draw(commands, args, compound=True, size=64)
    want = (1 - render.rasterize(commands, args, size=64))[:, None].expand(1, 3, 64, 64)
    assert (stroke - want).abs().max().item() <= 2.0 ** -22 and stroke.min().item() < 0.2


def test_order_matters(draw_ops):
    commands, args = ring()
    img = render.draw(commands.flip(1), args.flip(1), filling=torch.tensor([[2, 1]]), size=64)[0]
    hole, band, _, outside = ring_masks()
    assert bool((img[:, hole] == 0.0).all()), "an erase path below the fill must not open a hole"
    assert bool((img[:, band] == 0.0).all()) and bool((img[:, outside] == 1.0).all())


def two_squares():
    return icon(square(34, 98), square(66, 130))


def two_square_pixels():
    """(row, column) strictly inside the first square only, the overlap, the second only, neither"""
    return (12, 12), (20, 20), (28, 28), (4, 40)


def _check_two_colours(img):
    fma = lambda alpha, paint, canvas: canvas + alpha * (paint - canvas)          # exact for these dyadic values
    first, both, second, neither = two_square_pixels()
    for ch in range(3):
        red = fma(0.5, RED[ch], 1.0)
        assert img[ch][first] == red and img[ch][both] == fma(0.5, BLUE[ch], red)
        assert img[ch][second] == fma(0.5, BLUE[ch], 1.0) and img[ch][neither] == 1.0
    assert img[:, 20, 20].tolist() == [0.5, 0.25, 0.75]


def test_two_colours_at_half_opacity_follow_the_fmaf_chain(draw_ops):
    commands, args = two_squares()
    colors = torch.tensor([RED, BLUE])
    _check_two_colours(render.draw(commands, args, filling=torch.tensor([[1, 1]]), colors=colors, opacity=0.5, size=64)[0])
    per_icon = render.draw(commands, args, fill=True, colors=colors[None], opacity=torch.tensor([[0.5, 0.5]]), size=64)[0]
    _check_two_colours(per_icon)
    # tensors out of range are clamped, NaN reads as 0
    wild = render.draw(commands, args, fill=True, colors=torch.tensor([[7.0, float("nan"), -3.0], [0.0, 0.0, 1.0]]),
                       opacity=torch.tensor([0.5, 0.5]), size=64)[0]
    _check_two_colours(wild)


def test_outline_over_fill(draw_ops):
    (c, a) = square()
    commands, args = icon((c, a), (c, a))
    grey = 0.75
    img = render.draw(commands, args, filling=torch.tensor([[1, 0]]), colors=torch.tensor([[grey] * 3, [0.0] * 3]), size=64)[0]
    inside, edge, _ = square_masks()
    deep, _, _ = square_masks(lo=9, hi=23)
    _, _, far = square_masks(lo=7, hi=25)
    half = 1.0 + 0.5 * (grey - 1.0)
    line = half + 0.9 * (0.0 - half)          # stroke coverage 0.5 + (1.6 - 0) / 4 on the line
    for ch in img:
        assert bool((ch[deep] == grey).all()) and bool((ch[far] == 1.0).all())
        assert (ch[edge] - line).abs().max().item() <= layered_atol(64, 2)
    assert inside.sum() > deep.sum()


def test_other_filling_values_draw_as_outline(draw_ops):
    commands, args = ring()
    want = (1 - render.rasterize(commands, args, size=64))[:, None].expand(1, 3, 64, 64)
    plain = render.draw(commands, args, size=64)
    assert (plain - want).abs().max().item() <= 2.0 ** -22 and plain.min().item() < 0.2
    for values in ([0, 0], [3, -1], [7, 255]):
        assert torch.equal(render.draw(commands, args, filling=torch.tensor([values]), size=64), plain), values


def test_empty_groups_leave_the_background(draw_ops):
    commands, args = torch.full((2, 3, 6), float(EOS)), torch.full((2, 3, 6, 11), -1.0)
    img = render.draw(commands, args, filling=torch.tensor([[1, 2, 0]] * 2), background=(0.25, 0.5, 0.75), size=16)
    assert img.shape == (2, 3, 16, 16)
    assert torch.equal(img, torch.tensor([0.25, 0.5, 0.75]).view(1, 3, 1, 1).expand(2, 3, 16, 16))
    # and an empty group between two others is skipped, whatever its paint says
    (c, a) = square()
    commands, args = icon((c, a), (torch.full_like(c, float(EOS)), a), (c, a))
    colors = torch.tensor([RED, (float("nan"),) * 3, BLUE])
    img = render.draw(commands, args, filling=torch.tensor([[1, 2, 0]]), colors=colors, opacity=torch.tensor([1.0, float("nan"), 1.0]))
    two = render.draw(commands[:, ::2], args[:, ::2], filling=torch.tensor([[1, 0]]), colors=colors[::2])
    assert torch.equal(img, two)


def test_argument_errors(draw_ops):
    commands, args = ring()
    ok = dict(filling=torch.tensor([[1, 2]]), size=16)
    render.draw(commands, args, **ok)
    for bad in (dict(filling=torch.tensor([[1, 2, 0]])), dict(filling=torch.tensor([1, 2])), dict(filling=torch.tensor([[1.0, 2.0]])),
                dict(colors=torch.zeros(3, 3)), dict(colors=torch.zeros(2, 4)), dict(colors=torch.zeros(2, 2, 3)),
                dict(opacity=torch.ones(3)), dict(opacity=torch.ones(1, 2, 1)), dict(background=(1.0, 1.0)),
                dict(compound=True), dict(fill_rule="winding"), dict(fill_rule=None),
                dict(colors=[[0.0, 0.0, 1.5], [0.0, 0.0, 0.0]]), dict(colors=[[0.0, -0.1, 0.0], [0.0, 0.0, 0.0]]),
                dict(opacity=1.01), dict(opacity=float("nan")), dict(background=-0.5), dict(background=(0.0, 2.0, 0.0)),
                dict(background=float("inf"))):
        with pytest.raises(ValueError):
            render.draw(commands, args, **{**ok, **bad})
    with pytest.raises(ValueError):
        render.draw(commands, args[:, :1], size=16)
    with pytest.raises(ValueError):
        render.draw(commands[0, 0], args[0, 0], size=16)
    # [N, S] is read as G = 1
    one = render.draw(commands[:, 0], args[:, 0], filling=torch.tensor([[1]]), size=16)
    assert torch.equal(one, render.draw(commands[:, :1], args[:, :1], filling=torch.tensor([[[1]]]), size=16))
    assert not render.draw(commands.float(), args.float().requires_grad_(True), size=8).requires_grad


def test_palette():
    for G in (1, 2, 8, 31):
        p = render.palette(G)
        assert p.shape == (G, 3) and p.dtype == torch.float32 and 0.0 <= p.min().item() and p.max().item() <= 1.0
        assert len({tuple(row) for row in p.tolist()}) == G
        assert p.amin(1).max().item() < 0.5, "a colour too pale to read on white paper"
    d = torch.cdist(render.palette(8), render.palette(8)) + torch.eye(8)
    assert d.min().item() > 0.2


def random_paint(B, G, seed):
    gen = torch.Generator().manual_seed(seed)
    modes = torch.randint(0, 3, (B, G), generator=gen, dtype=torch.int32)
    paint = torch.rand(B, G, 4, generator=gen)
    paint[..., 3] = 0.3 + 0.7 * paint[..., 3]
    return modes, paint, torch.rand(3, generator=gen).tolist()


@pytest.mark.parametrize("compound", [None, "fill", "stroke"])
@pytest.mark.parametrize("evenodd", [False, True])
@pytest.mark.parametrize("n", [2, 10])
def test_fp32_formulas_stay_within_their_share_of_the_bound(n, evenodd, compound):
    from tests.test_metrics_gpu import _random_sequences
    commands, args = _random_sequences(3, 4, 12, seed=5 + n)
    c, a = commands.reshape(12, 12), args.reshape(12, 12, 11)
    modes, paint, background = random_paint(3, 4, seed=n)
    kw = dict(background=background, evenodd=evenodd, compound=compound, n=n, groups=4, as_double=True)
    m = None if compound else modes
    layers = 1 if compound else 3             # (group 3 of _random_sequences is empty)
    for size in (8, 64, 100):
        want = LR.draw(c, a, m, paint, size=size, **kw)
        got = LR.draw(c, a, m, paint, size=size, dtype=torch.float32, **kw)
        assert got.dtype == torch.float32 and want.dtype == torch.float64
        s = 256.0 / size
        err = (got.double() - want).abs().max().item()
        print(f"fp32 against float64, n={n} evenodd={evenodd} compound={compound} size={size}: max err {err:.3e} = {err * s:.3e} / s")
        assert err <= layers * (FP32_ATOL / s + 2.0 ** -22)
        assert 0.0 < want.mean().item() < 1.0


def test_binding_declares_the_layered_entry_points():
    for name in ("dsvg_raster_segments_layers", "dsvg_raster_sweep_layers"):
        assert name in lib.SIGNATURES
    assert lib.DSVG_LAYER_FILL == LR.FILL and lib.DSVG_LAYER_ERASE == LR.ERASE and lib.DSVG_LAYER_OUTLINE == LR.OUTLINE
    assert "draw" in render.__all__ and "palette" in render.__all__
