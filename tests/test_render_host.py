"""deepsvg_amd.render on CPU: the float64 restatement of what an image is (tests/raster_ref.py) on cases whose images are
known in closed form, and the host logic of rasterize / reconstruction_images / interpolate with the three raster ops
replaced by the restatement.

Tolerance against the restatement, in ink units: 2 * DIST_ATOL / s with DIST_ATOL = 1e-3 argument units and s = 256 / size
the pixel pitch.  A chord vertex carries at most POINT_ATOL = 5e-4 (the bound of tests/test_metrics_host.py: a coefficient
sum of the cubic reaches 8 * 255 ~ 2048, half an fp32 ulp there is 1.2e-4, four such terms), which is also the Hausdorff
bound on the chord between two such vertices.  The closest point a + t (b - a) and the difference q = p - (a + t (b - a)) add
a few fp32 ulps at magnitude 512 (pixel centres and vertices within 0..256, differences within 512), about 2.4e-4; the
distance is the cancellation-free form of include/dsvg.h, for which this holds.  5e-4 + 2.4e-4, rounded up: 1e-3.  Ink is
d / s; the factor 2 covers a pixel whose inside test is decided by rounding: the two fill branches meet at d = 0, so such a
pixel moves by at most 2 d / s with d <= DIST_ATOL.  No pixel is excluded.
Checked on CPU (test_fp32_formulas_stay_within_their_share_of_the_tolerance): the same formulas in fp32 against float64, on
the same float64 chord lists, stay below FP32_ATOL / s with FP32_ATOL = 4.4e-5 - random icons from the command pool of
tests/test_metrics_gpu.py::_random_sequences, arguments -1..255, sizes 8, 64 and 100, n = 2 and 10, both modes (largest seen
here: 1.9e-5 / s) - well inside the 2.4e-4 the derivation grants the arithmetic, so the bound has real margin."""
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import lib, render
from tests import helpers as H
from tests import raster_ref as RR

POINT_ATOL, DIST_ATOL, FP32_ATOL = 5e-4, 1e-3, 4.4e-5
M, L_, C_, A_, EOS, SOS, Z_ = 0, 1, 2, 3, 4, 5, 6


def ink_atol(size):
    return 2 * DIST_ATOL / (256.0 / size)


@pytest.fixture
def raster_ops(emulated_ops):
    saved = RR.install()
    yield
    RR.restore(saved)


def sequence(rows, length=None):
    """rows of (command, end x, end y) -> commands f32 [1, L], args f32 [1, L, 11]; every other argument is -1, rows past the
    list are EOS with -1 everywhere"""
    length = length or len(rows)
    commands = torch.full((1, length), float(EOS))
    args = torch.full((1, length, 11), -1.0)
    for i, (c, x, y) in enumerate(rows):
        commands[0, i] = c
        args[0, i, 9], args[0, i, 10] = x, y
    return commands, args


def square(lo=34, hi=98, reverse=False, length=8):
    corners = [(hi, lo), (hi, hi), (lo, hi), (lo, lo)]
    if reverse:
        corners = [(lo, hi), (hi, hi), (hi, lo), (lo, lo)]
    return sequence([(M, lo, lo)] + [(L_, x, y) for x, y in corners], length)


def square_masks(size=64, lo=8, hi=24):
    """pixel classes of the square with corners (34, 34) and (98, 98) at size 64 (s = 4: the centres of rows / columns 8 and
    24 sit on the edges): strictly inside, on the outline, strictly outside"""
    i = torch.arange(size)
    r, c = i.view(-1, 1), i.view(1, -1)
    inside = (r > lo) & (r < hi) & (c > lo) & (c < hi)
    within = (r >= lo) & (r <= hi) & (c >= lo) & (c <= hi)
    return inside, within & ~inside, ~within


def test_filled_square_is_one_inside_zero_outside_half_on_the_edge(raster_ops):
    commands, args = square()
    img = render.rasterize(commands, args, size=64, fill=True)[0]
    inside, edge, outside = square_masks()
    assert img.shape == (64, 64) and img.dtype == torch.float32
    assert bool((img[inside] == 1.0).all()) and bool((img[outside] == 0.0).all())
    err = (img[edge] - 0.5).abs().max().item()
    print(f"filled square: edge pixels off 0.5 by {err:.3e}")
    assert err <= ink_atol(64) and int(edge.sum()) == 64


def test_stroked_square_is_point_nine_on_the_line_and_zero_a_pixel_away(raster_ops):
    commands, args = square()
    img = render.rasterize(commands, args, size=64, stroke_width=3.2)[0]
    _, edge, _ = square_masks()
    _, _, far = square_masks(lo=7, hi=25)
    near_inside, _, _ = square_masks(lo=9, hi=23)
    err = (img[edge] - 0.9).abs().max().item()
    print(f"stroked square: line pixels off 0.9 by {err:.3e}")
    assert err <= ink_atol(64)
    assert bool((img[far] == 0).all()) and bool((img[near_inside] == 0).all()) and bool((img[9, 9:24] == 0).all())


def test_a_sequence_that_starts_with_a_drawing_command_starts_at_the_origin(raster_ops):
    commands, args = sequence([(L_, 128, 128)], length=3)
    chords = RR.chord_list(commands, args, n=2)[0]
    assert chords["a"].tolist() == [[0.0, 0.0]] and chords["b"].tolist() == [[128.0, 128.0]]
    img = render.rasterize(commands, args, size=64, n=2)[0]
    d = torch.arange(64)
    assert (img[d[:32], d[:32]] - 0.9).abs().max().item() <= ink_atol(64)       # the diagonal up to (128, 128) ...
    assert bool((img[d[34:], d[34:]] == 0).all())                               # ... and not beyond


@pytest.mark.parametrize("fill", [False, True])
def test_rows_that_do_not_draw_still_supply_start_points(raster_ops, fill):
    want_c, want_a = sequence([(M, 50, 10), (L_, 50, 90), (L_, 120, 90)], length=6)
    want = render.rasterize(want_c, want_a, fill=fill)
    for other in (M, A_, Z_, SOS, EOS):
        commands, args = sequence([(M, 200, 200), (other, 50, 10), (L_, 50, 90), (L_, 120, 90)], length=6)
        chords = RR.chord_list(commands, args, n=10, fill=fill)[0]
        assert len(chords["seq"]) == 2 * 9 + int(fill) and chords["a"][0].tolist() == [50.0, 10.0]
        assert torch.equal(render.rasterize(commands, args, fill=fill), want), other
    # a padding row (EOS with -1 everywhere) supplies (-1, -1)
    commands, args = sequence([(EOS, -1, -1), (L_, 100, 100)], length=4)
    assert RR.chord_list(commands, args, n=2)[0]["a"].tolist() == [[-1.0, -1.0]]
    # and an `a` row draws nothing by itself
    commands, args = sequence([(M, 10, 10), (A_, 200, 200), (EOS, -1, -1)])
    assert bool((render.rasterize(commands, args, fill=fill) == 0).all())


def test_an_open_sub_path_of_one_chord_fills_nothing(raster_ops):
    commands, args = sequence([(M, 30, 30), (L_, 200, 180)], length=4)
    chords = RR.chord_list(commands, args, n=2, fill=True)[0]
    assert len(chords["seq"]) == 2 and chords["back"].tolist() == [0, 1]
    d, inside = RR.image(chords["a"], chords["b"], chords["seq"], 64, fill=True, return_distance=True)
    assert not bool(inside.any())
    img = render.rasterize(commands, args, size=64, fill=True, n=2)[0]
    assert img.max().item() <= 0.5 and torch.equal(img, (0.5 - d / 4).clamp(0, 1).float())


def test_two_sequences_overlap_as_a_union(raster_ops):
    """of opposite orientation: in ONE winding count the overlap would cancel to 0"""
    (c1, a1), (c2, a2) = square(34, 98), square(66, 130, reverse=True)
    commands, args = torch.stack([c1[0], c2[0]])[None], torch.stack([a1[0], a2[0]])[None]          # (1, 2, S)
    img = render.rasterize(commands, args, size=64, fill=True)[0]
    assert img[20, 20] == 1.0 and img[12, 12] == 1.0 and img[28, 28] == 1.0 and img[12, 28] == 0.0 and img[4, 4] == 0.0
    one = render.rasterize(torch.cat([c1[:, :5], c2], 1), torch.cat([a1[:, :5], a2], 1), size=64, fill=True)[0]
    assert one[12, 12] == 1.0 and one[28, 28] == 1.0
    assert one[20, 20] == 0.0, "the same chords as one sequence: +1 and -1 cancel in the overlap"


def test_a_self_intersecting_sub_path_follows_non_zero_not_even_odd(raster_ops):
    """a square walked around twice winds 2 around its interior: non-zero fills it, even-odd would not"""
    corners = [(98, 34), (98, 98), (34, 98), (34, 34)]
    commands, args = sequence([(M, 34, 34)] + [(L_, x, y) for x, y in corners * 2], length=10)
    img = render.rasterize(commands, args, size=64, fill=True)[0]
    inside, _, outside = square_masks()
    assert bool((img[inside] == 1.0).all()) and bool((img[outside] == 0.0).all())
    # and the pentagram: its centre has winding 2
    star = [(128 + 100 * torch.sin(torch.tensor(k * 4 * torch.pi / 5)).item(),
             128 - 100 * torch.cos(torch.tensor(k * 4 * torch.pi / 5)).item()) for k in range(6)]
    commands, args = sequence([(M, *star[0])] + [(L_, x, y) for x, y in star[1:]], length=8)
    assert render.rasterize(commands, args, size=64, fill=True)[0, 32, 32] == 1.0


def _random_icons(N=3, G=4, S=12, seed=3):
    gen = torch.Generator().manual_seed(seed)
    pool = torch.tensor([0, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6])
    return pool[torch.randint(0, len(pool), (N, G, S), generator=gen)], torch.randint(-1, 256, (N, G, S, 11), generator=gen)


def test_rasterize_shapes_and_dtypes(raster_ops):
    commands, args = _random_icons()
    N, G, S = commands.shape
    icons = render.rasterize(commands, args, size=32)
    rows = render.rasterize(commands.reshape(N * G, S), args.reshape(N * G, S, 11), size=32)
    assert icons.shape == (N, 32, 32) and rows.shape == (N * G, 32, 32) and icons.dtype == torch.float32
    # stroke ink falls with the distance, and the distance to an icon is the least over its groups
    assert torch.equal(icons, rows.view(N, G, 32, 32).amax(1))
    assert torch.equal(render.rasterize(commands[:, :1], args[:, :1], size=32), rows.view(N, G, 32, 32)[:, 0])
    for fill in (False, True):
        as_int = render.rasterize(commands, args, size=32, fill=fill)
        as_float = render.rasterize(commands.float(), args.float(), size=32, fill=fill)
        assert torch.equal(as_int, as_float)
        assert torch.equal(render.rasterize(commands.int(), args.float(), size=32, fill=fill), as_int)       # mixed: read as float
    assert not render.rasterize(commands.float(), args.float().requires_grad_(True), size=8).requires_grad
    with pytest.raises(ValueError):
        render.rasterize(torch.zeros(4), torch.zeros(4, 11))
    with pytest.raises(ValueError):
        render.rasterize(torch.zeros(2, 4), torch.zeros(2, 5, 11))


def test_emulated_segments_and_sweep_agree_with_the_direct_restatement(raster_ops):
    from deepsvg_amd import ops
    commands, args = _random_icons()
    N, G, S = commands.shape
    c, a = commands.reshape(N * G, S), args.reshape(N * G, S, 11)
    for fill in (False, True):
        segs, counts = ops.raster_segments(c, a, n=7, groups=G, fill=fill)
        assert segs.shape == (N, G * (S * 6 + (S + 1) // 2 * int(fill)), 5) and counts.dtype == torch.int32
        got = ops.raster_sweep(segs, counts, size=32, fill=fill)
        want = RR.rasterize(c, a, size=32, fill=fill, n=7, groups=G)
        err = (got - want).abs().max().item()
        print(f"records -> image against chord list -> image, fill={fill}: {err:.3e}")
        assert err <= ink_atol(32)


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("n", [2, 10])
def test_fp32_formulas_stay_within_their_share_of_the_tolerance(n, fill):
    from tests.test_metrics_gpu import _random_sequences
    commands, args = _random_sequences(3, 4, 12, seed=5 + n)
    lists = RR.chord_list(commands.reshape(12, 12), args.reshape(12, 12, 11), n, 4, fill)
    assert all(len(ch["seq"]) for ch in lists)
    for size in (8, 64, 100):
        err = max((RR.image(ch["a"], ch["b"], ch["seq"], size, 3.2, fill, dtype=torch.float32).double()
                   - RR.image(ch["a"], ch["b"], ch["seq"], size, 3.2, fill)).abs().max().item() for ch in lists)
        s = 256.0 / size
        print(f"fp32 against float64, n={n} fill={fill} size={size}: max ink err {err:.3e} = {err * s:.3e} / s")
        assert err <= FP32_ATOL / s


def _model(name):
    g, cfg, commands, args, _ = H.golden_setup(name)
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(H.weights_for(model, g["wseed"]))
    return model, commands, args


@pytest.mark.parametrize("training", [False, True])
def test_reconstruction_images_host_logic(raster_ops, training):
    model, commands, args = _model("onestage50_n3")
    model.train(training)
    seen = {}
    greedy = model.greedy_sample

    def spy(*a, **k):
        seen["kw"], seen["training"] = k, model.training
        seen["out"] = greedy(*a, **k)
        return seen["out"]
    model.greedy_sample = spy
    res = render.reconstruction_images(model, commands, args, size=32, fill=True)
    assert model.training == training and seen["training"] is False
    assert seen["kw"] == dict(label=None, concat_groups=False, temperature=0.0)
    N = commands.shape[0]
    assert res["decoded"].shape == (N, 32, 32) and res["target"].shape == (N, 32, 32)
    assert torch.equal(res["decoded"], render.rasterize(*seen["out"], size=32, fill=True))
    assert torch.equal(res["target"], render.rasterize(commands, args, size=32, fill=True)) and bool(res["target"].any())
    # decoding replaced by the targets: the two outputs are equal
    model.greedy_sample = lambda *a, **k: (commands.long(), args.long())
    res = render.reconstruction_images(model, commands, args, size=32)
    assert torch.equal(res["decoded"], res["target"]) and model.training == training


@pytest.mark.parametrize("name", ["hier_ordered_n5", "onestage50_n3"])
def test_interpolate_host_logic(raster_ops, name):
    model, commands, args = _model(name)
    model.train()
    with torch.no_grad():
        z = model(commands, args, None, None, encode_mode=True)                  # seq-first (1, 1, N, dim_z)
    N = z.shape[2]
    z1, z2 = z, z.flip(2)
    seen = {}
    greedy = model.greedy_sample

    def spy(*a, **k):
        seen["z"], seen["calls"] = k["z"], seen.get("calls", 0) + 1
        return greedy(*a, **k)
    model.greedy_sample = spy
    res = render.interpolate(model, z1, z2, steps=3, size=32)
    assert seen["calls"] == 1 and model.training
    assert res["frames"].shape == (N, 3, 32, 32) and res["frames"].dtype == torch.float32
    assert res["commands"].shape[:2] == (N, 3) and res["args"].shape[:2] == (N, 3) and res["args"].shape[-1] == 11
    assert torch.equal(res["frames"], render.rasterize(res["commands"].flatten(0, 1), res["args"].flatten(0, 1),
                                                       size=32).view(N, 3, 32, 32))
    # the ends are the icons of z1 and z2 decoded alone
    for frame, zz in ((0, z1), (2, z2)):
        with torch.no_grad():
            model.eval()
            cy, ay = greedy(None, None, None, None, z=zz.permute(2, 1, 0, 3), concat_groups=False, temperature=0.0)
            model.train()
        assert torch.equal(res["commands"][:, frame], cy) and torch.equal(res["args"][:, frame], ay)
        assert torch.equal(res["frames"][:, frame], render.rasterize(cy, ay, size=32))
    # both layouts of z give the same frames
    bf = render.interpolate(model, z1.permute(2, 1, 0, 3), z2.permute(2, 1, 0, 3), steps=3, size=32)
    assert torch.equal(bf["frames"], res["frames"]) and torch.equal(bf["commands"], res["commands"])
    # the alphas: linspace without ease, t^2 / (2 (t^2 - t) + 1) with it
    render.interpolate(model, z1, z2, steps=5, ease=False, size=8)
    a = torch.linspace(0, 1, 5).view(1, 5, 1)
    flat1, flat2 = z1.reshape(N, 1, -1), z2.reshape(N, 1, -1)
    assert torch.equal(seen["z"], ((1 - a) * flat1 + a * flat2).reshape(N * 5, 1, 1, -1))
    assert torch.equal(render.interpolation_alphas(5, ease=False), torch.linspace(0, 1, 5))
    t = torch.linspace(0, 1, 5)
    eased = render.interpolation_alphas(5)
    assert torch.allclose(eased, t ** 2 / (2 * (t ** 2 - t) + 1)) and eased[0] == 0 and eased[-1] == 1 and eased[2] == 0.5
    with pytest.raises(ValueError):
        render.interpolate(model, z1, z2[:, :, :1], steps=3)


def test_binding_declares_the_raster_entry_points():
    assert lib.ABI_VERSION >= 16
    for name in ("dsvg_raster_workspace_bytes", "dsvg_raster_segments", "dsvg_raster_sweep"):
        assert name in lib.SIGNATURES
