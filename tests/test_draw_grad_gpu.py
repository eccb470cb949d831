"""The gradient of deepsvg_amd.render.draw on a real MI355X: dsvg_raster_sweep_layers_nn, dsvg_raster_blend_bwd,
dsvg_raster_sweep_layers_bwd and dsvg_raster_segments_layers_bwd (csrc/raster.hip) against the float64 restatement of
tests/raster_layers_grad_ref.py, their exactness properties, and draw_with_grad / picture_loss / refine_to_pictures end to end.
Every test prints the largest error it saw before it asserts.

Tolerances (tests/test_draw_grad_host.py and tests/test_render_grad_host.py derive and measure them on the same inputs): the
blend backward against the restatement fed the kernel's own coverage: dcov 4 * BLEND_SPREAD * max |dout|, dpaint 4 * PAINT_SPREAD
* max |dout| * the pixels of an image; the chord backward 4 * sweep_spread(live d) * max |dcov| against the restatement fed the kernel's own
records, coverage, arg-min and dcov: SPREAD itself on the cases whose smallest live distance is >= MIN_LIVE_D (SWEEP_CASES;
asserted here), SPREAD * MIN_LIVE_D / live d on `g8_s100` and `long`, which cannot hold that margin (derived and measured in the
host file);
the segment backward 4 * SEG_SPREAD * max |dsegs|; the arg-min is checked by distance (DIST_ATOL of tests/test_render_host.py).
The end-to-end fixture and its margins are e2e_layers / test_layered_fixture_margins of the host file: with them the float64
restatement runs from the ARGUMENTS with its own coverage and its own arg-min.  No pixel is excluded anywhere."""
import pytest
import torch

from deepsvg_amd import lib, ops, render
from tests import raster_grad_ref as RG
from tests import raster_layers_grad_ref as LG
from tests import raster_layers_ref as LR
from tests.poison import three_runs
from tests.test_draw_grad_host import (BLEND_CASES, BLEND_SPREAD, E2E_G, E2E_N, E2E_SIZE, PAINT_SPREAD, SWEEP_CASES, blend_case,
                                       blend_dout, e2e_layers, shifted_ring, smallest_live_distance, sweep_spread)
from tests.test_render_gpu import LDS_CHORDS
from tests.test_render_grad_host import MIN_LIVE_D, SEG_CASES, SEG_N, SEG_SPREAD, SPREAD, case_commands
from tests.test_render_host import DIST_ATOL, ink_atol

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [*BLEND_CASES, "long"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _compound(kw):
    return kw["compound"]


@pytest.fixture(scope="module")
def forwards():
    """per case, computed once and left unchanged: the inputs on the device, the kernel's records and tables, and the forward
    twin's picture, coverage and arg-min (cull off)"""
    cache = {}

    def get(name):
        if name not in cache:
            commands, args, modes, paint, background, kw = blend_case(name)
            c, a, p = commands.to(DEV), args.to(DEV), paint.to(DEV)
            m = None if modes is None else modes.to(DEV)
            if _compound(kw):
                segs, counts = ops.raster_segments(c, a, n=kw["n"], groups=kw["groups"], fill=True)
                first = None
            else:
                segs, counts, first = ops.raster_segments_layers(c, a, m, n=kw["n"], groups=kw["groups"])
            draw = dict(background=background, size=kw["size"], evenodd=kw["evenodd"], compound=_compound(kw))
            out, cov, idx = ops.raster_sweep_layers_nn(segs, counts, first, m, p, cull=False, **draw)
            cache[name] = dict(c=c, a=a, modes=m, paint=p, background=background, kw=kw, draw=draw, segs=segs, counts=counts,
                               first=first, out=out, cov=cov, idx=idx)
        return cache[name]
    return get


def _host(f, *keys):
    return [None if f[k] is None else f[k].cpu() for k in keys]


# ---- the forward twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_twin_keeps_the_picture_and_names_a_nearest_chord_of_the_layer(gpu_device, forwards, name):
    f = forwards(name)
    kw, size = f["kw"], f["kw"]["size"]
    tables = (f["segs"], f["counts"], f["first"], f["modes"], f["paint"])
    want = ops.raster_sweep_layers(*tables, cull=False, **f["draw"])
    NL = 1 if _compound(kw) else kw["groups"]
    for cull in (False, True):
        out, cov, idx = ops.raster_sweep_layers_nn(*tables, cull=cull, **f["draw"])
        assert out.dtype == cov.dtype == torch.float32 and idx.dtype == torch.int32
        assert cov.shape == idx.shape == (out.shape[0], NL, size, size) and out.shape == (out.shape[0], 3, size, size)
        assert torch.equal(_bits(out), _bits(want)), "raster_sweep_layers_nn changed the picture"
        assert torch.equal(_bits(out), _bits(ops.raster_sweep_layers(*tables, cull=cull, **f["draw"])))
        assert torch.equal(_bits(cov), _bits(f["cov"])) and torch.equal(idx, f["idx"]), "culling or a second run changed cov / idx"
        live = (cov > 0) & (cov < 1)
        assert torch.equal(idx == -1, ~live), "idx is -1 exactly where the coverage is 0 or 1"
        assert float(cov.min()) >= 0.0 and float(cov.max()) <= 1.0
    L = f["c"].shape[1]
    pic = render.draw(f["c"].view(-1, kw["groups"], L), f["a"].view(-1, kw["groups"], L, 11),
                      filling=None if _compound(kw) else f["modes"], colors=f["paint"][..., :3], opacity=f["paint"][..., 3],
                      background=f["background"], size=size, n=kw["n"], compound=bool(_compound(kw)), fill=bool(_compound(kw)),
                      fill_rule="evenodd" if kw["evenodd"] else "nonzero")
    assert torch.equal(_bits(pic), _bits(want)), "the twin's picture is not draw's"
    segs, counts, first, modes, cov, idx = _host(f, "segs", "counts", "first", "modes", "cov", "idx")
    worst = worst_cov = 0.0
    n_live = n_layers = 0
    for i in range(segs.shape[0]):
        a, b = LG._records64(segs[i], counts[i])
        ranges = LG.layer_ranges(None if first is None else first[i], counts[i], NL, _compound(kw))
        mode = LG.layer_modes(None if modes is None else modes[i], NL, _compound(kw))
        for g, (lo, hi) in enumerate(ranges):
            sel = idx[i, g] >= 0
            if hi == lo:
                assert bool((cov[i, g] == 0).all()) and not bool(sel.any()), "a layer without chords has cov 0 and idx -1"
                continue
            n_layers += 1
            assert bool(((idx[i, g] >= lo) & (idx[i, g] < hi))[sel].all()), "the named chord is not one of the pixel's layer"
            want_cov = LR.coverage(a[lo:hi], b[lo:hi], mode[g], size, 3.2, kw["evenodd"])
            worst_cov = max(worst_cov, (cov[i, g].double() - want_cov).abs().max().item())
            if bool(sel.any()):
                n_live += int(sel.sum())
                dmin, _ = RG.nearest(a[lo:hi], b[lo:hi], size)
                worst = max(worst, (RG.distance_to(a, b, idx[i, g].long(), size) - dmin)[sel].max().item())
    print(f"raster_sweep_layers_nn `{name}` size={size}: {n_layers} layers with chords, {n_live} live pixels; the named chord is at "
          f"most {worst:.3e} farther than the float64 nearest of its layer (bound {DIST_ATOL:.1e}); coverage max err "
          f"{worst_cov:.3e} (bound {ink_atol(size):.3e})")
    assert n_live > 0 and worst <= DIST_ATOL and worst_cov <= ink_atol(size)
    if name == "gaps_s33":
        assert int(counts[1]) == 0 and bool((f["out"][1] == torch.tensor(f["background"], device=DEV).view(3, 1, 1)).all())
        assert first[0, 1] == first[0, 2] and first[0, 1] > 0 and first[0, 2] < counts[0], "an empty group between two drawn ones"
    if name == "g3_s33":
        assert 7 in modes.flatten().tolist()
    if name == "long":
        ends = first[:, 1:]
        assert int(counts.min()) > LDS_CHORDS
        assert bool(((ends % LDS_CHORDS != 0) & (ends < counts.view(-1, 1))).any()), "no layer ends inside a chord tile"
        spans = (first[:, :-1] // LDS_CHORDS) != ((first[:, 1:] - 1) // LDS_CHORDS)
        assert bool((spans & (first[:, 1:] > first[:, :-1])).any()), "no layer runs across two chord tiles"


# ---- the blend backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_blend_bwd_matches_the_restatement(gpu_device, forwards, name):
    f = forwards(name)
    kw, size = f["kw"], f["kw"]["size"]
    dout = blend_dout(name, f["out"].shape).to(DEV)
    call = (f["cov"], f["counts"], f["first"], f["modes"], f["paint"])
    extra = dict(background=f["background"], compound=_compound(kw))
    cap = f["segs"].shape[1]
    dcov, dpaint = ops.raster_blend_bwd(*call, dout, cap, **extra)
    assert dcov.shape == f["cov"].shape and dpaint.shape == f["paint"].shape and dcov.dtype == dpaint.dtype == torch.float32
    again = ops.raster_blend_bwd(*call, dout, cap, **extra)
    assert torch.equal(_bits(dcov), _bits(again[0])) and torch.equal(_bits(dpaint), _bits(again[1])), "two runs differ in bits"
    zero = ops.raster_blend_bwd(*call, torch.zeros_like(dout), cap, **extra)
    assert bool((zero[0] == 0).all()) and bool((zero[1] == 0).all()), "dout = 0 does not give exact zeros"
    cov, counts, first, modes, paint = _host(f, "cov", "counts", "first", "modes", "paint")
    want_cov, want_paint = LG.raster_blend_bwd(cov, counts, first, modes, paint, dout.cpu(), cap, as_double=True, **extra)
    scale = dout.abs().max().item()
    got_cov, got_paint = dcov.cpu(), dpaint.cpu()
    assert bool(torch.isfinite(got_cov).all()) and bool(torch.isfinite(got_paint).all())
    err_cov = (got_cov.double() - want_cov).abs().max().item() / scale
    err_paint = (got_paint.double() - want_paint).abs().max().item() / (scale * size * size)
    print(f"raster_blend_bwd `{name}` size={size}: dcov max err {err_cov:.3e} of max |dout| (bound {4 * BLEND_SPREAD:.1e}), dpaint max "
          f"err {err_paint:.3e} of max |dout| x pixels (bound {4 * PAINT_SPREAD:.1e}); max |dcov| {want_cov.abs().max().item():.3e}, "
          f"max |dpaint| {want_paint.abs().max().item():.3e}")
    assert bool(want_cov.any()) and bool(want_paint.any())
    assert err_cov <= 4 * BLEND_SPREAD and err_paint <= 4 * PAINT_SPREAD
    assert bool((got_cov[want_cov == 0] == 0).all()) and bool((got_paint[want_paint == 0] == 0).all()), "a structural zero is not exact"


def test_blend_bwd_gives_clamped_erase_and_skipped_paint_exact_zeros(gpu_device, forwards):
    f = forwards("gaps_s33")
    paint = f["paint"].clone()
    paint[0, 0, 0], paint[0, 0, 1], paint[0, 0, 3], paint[2, 1, 3], paint[2, 2, 2] = 1.5, float("nan"), 1.0, -0.5, -1e-3
    out, cov, idx = ops.raster_sweep_layers_nn(f["segs"], f["counts"], f["first"], f["modes"], paint, **f["draw"])
    dout = blend_dout("clamped", out.shape).to(DEV)
    dcov, dpaint = ops.raster_blend_bwd(cov, f["counts"], f["first"], f["modes"], paint, dout, f["segs"].shape[1],
                                        background=f["background"])
    want_cov, want_paint = LG.raster_blend_bwd(cov.cpu(), f["counts"].cpu(), f["first"].cpu(), f["modes"].cpu(), paint.cpu(),
                                               dout.cpu(), f["segs"].shape[1], background=f["background"], as_double=True)
    got = dpaint.cpu()
    err = (got.double() - want_paint).abs().max().item() / (dout.abs().max().item() * 33 * 33)
    print(f"raster_blend_bwd with clamped paint: dpaint max err {err:.3e} of max |dout| x pixels (bound {4 * PAINT_SPREAD:.1e})")
    assert err <= 4 * PAINT_SPREAD and bool((got[want_paint == 0] == 0).all())
    assert got[0, 0, 0] == 0 and got[0, 0, 1] == 0 and got[2, 1, 3] == 0 and got[2, 2, 2] == 0, "clamped or NaN paint"
    assert got[0, 0, 3] != 0 and got[0, 0, 2] != 0, "a value ON the clamp passes the gradient"
    modes = f["modes"].cpu()
    assert bool((got[..., :3][modes == 2] == 0).all()) and bool((got[1] == 0).all()) and bool((got[0, 1] == 0).all())
    assert bool(torch.isfinite(dcov).all())


# ---- the chord backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_sweep_layers_bwd_matches_the_restatement(gpu_device, forwards, name):
    f = forwards(name)
    kw, size = f["kw"], f["kw"]["size"]
    dout = blend_dout(name, f["out"].shape).to(DEV)
    dcov, _ = ops.raster_blend_bwd(f["cov"], f["counts"], f["first"], f["modes"], f["paint"], dout, f["segs"].shape[1],
                                   background=f["background"], compound=_compound(kw))
    call = (f["segs"], f["counts"], f["first"], f["modes"], f["cov"], f["idx"])
    below = (torch.arange(f["segs"].shape[1], device=DEV).view(1, -1) < f["counts"].view(-1, 1)).unsqueeze(-1)
    results = []
    for wide in (False, True):
        got = ops.raster_sweep_layers_bwd(*call, dcov, compound=_compound(kw), wide=wide)
        assert got.shape == (f["segs"].shape[0], f["segs"].shape[1], 4) and got.dtype == torch.float32
        again = ops.raster_sweep_layers_bwd(*call, dcov, compound=_compound(kw), wide=wide)
        assert torch.equal(_bits(torch.where(below, got, 0)), _bits(torch.where(below, again, 0))), "two runs differ in bits"
        zero = ops.raster_sweep_layers_bwd(*call, torch.zeros_like(dcov), compound=_compound(kw), wide=wide)
        assert bool((torch.where(below, zero, 0) == 0).all()), "dcov = 0 does not give exact zeros"
        results.append(torch.where(below, got, 0).cpu())
        assert bool(torch.isfinite(results[-1]).all())
    segs, counts, first, modes, cov, idx = _host(f, "segs", "counts", "first", "modes", "cov", "idx")
    want = LG.raster_sweep_layers_bwd(segs, counts, first, modes, cov, idx, dcov.cpu(), compound=_compound(kw), as_double=True)
    live_d = smallest_live_distance(segs, counts, cov, idx)
    scale = dcov.abs().max().item()
    err = max((got.double() - want).abs().max().item() for got in results) / scale
    assert live_d > 0
    print(f"raster_sweep_layers_bwd `{name}` size={size}: max err {err:.3e} of max |dcov| (bound {4 * sweep_spread(live_d):.1e}); "
          f"smallest live d {live_d:.3e}, max |dsegs| {want.abs().max().item():.3e}")
    assert bool(want.any())
    named = torch.zeros(want.shape[:2], dtype=torch.bool)
    for i in range(segs.shape[0]):
        named[i, idx[i][idx[i] >= 0].long()] = True
    for got in results:
        assert bool((got[~named] == 0).all()), "a record no pixel names did not get exact zeros"
    assert err <= 4 * sweep_spread(live_d)
    if name in SWEEP_CASES:
        assert live_d >= MIN_LIVE_D and sweep_spread(live_d) == SPREAD


# ---- the segment backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SEG_N)
@pytest.mark.parametrize("G,L", SEG_CASES)
def test_segments_layers_bwd_matches_the_restatement(gpu_device, G, L, n):
    commands = case_commands(G, L, seed=G + L + n)
    B = commands.shape[0] // G
    gen = torch.Generator().manual_seed(G + n)
    modes = torch.tensor([0, 1, 2, 7], dtype=torch.int32)[torch.randint(0, 4, (B, G), generator=gen)]
    if G > 1:
        modes[:, 0], modes[:, 1] = 1, 0                     # (mixed in every icon)
    c, m = commands.to(DEV), modes.to(DEV)
    segs, counts, first = ops.raster_segments_layers(c, torch.zeros(*c.shape, 11, device=DEV), m, n=n, groups=G)
    want_counts = [sum(ly["a"].shape[0] for ly in icon)
                   for icon in LR.group_chords(commands, torch.zeros(*commands.shape, 11), modes.tolist(), n, G)]
    assert counts.tolist() == want_counts
    dsegs = torch.randn(B, segs.shape[1], 4, generator=gen)
    want = LG.raster_segments_layers_bwd(commands, dsegs, counts.cpu(), modes, n=n, groups=G, as_double=True)
    d = dsegs.to(DEV)
    dargs = torch.full((*commands.shape, 11), float("nan"), device=DEV)
    lib.check(lib.load().dsvg_raster_segments_layers_bwd(c.data_ptr(), d.data_ptr(), counts.data_ptr(), m.data_ptr(), B, G, L, n,
                                                         dargs.data_ptr(), None), "dsvg_raster_segments_layers_bwd")
    got = dargs.cpu()
    assert bool(torch.isfinite(got).all()), "an element was not written"
    err = (got.double() - want).abs().max().item() / dsegs.abs().max().item()
    print(f"raster_segments_layers_bwd G={G} L={L} n={n}: max err {err:.3e} of max |dsegs| (bound {4 * SEG_SPREAD:.1e})")
    assert err <= 4 * SEG_SPREAD and bool(want.any())
    assert bool((got[want == 0] == 0).all()), "a structural zero is not exact"
    assert torch.equal(_bits(ops.raster_segments_layers_bwd(c, d, counts, m, n=n, groups=G).cpu()), _bits(got))
    assert bool((ops.raster_segments_layers_bwd(c, torch.zeros_like(d), counts, m, n=n, groups=G) == 0).all()), \
        "dsegs = 0 does not give exact zeros"
    # with one mode for every group it is raster_segments_bwd, bit for bit
    for mode, fill in ((0, False), (1, True)):
        uniform = torch.full_like(m, mode)
        k = ops.raster_segments(c, torch.zeros(*c.shape, 11, device=DEV), n=n, groups=G, fill=fill)[1]
        one = ops.raster_segments_layers_bwd(c, d, k, uniform, n=n, groups=G)
        if fill:
            assert torch.equal(_bits(one), _bits(ops.raster_segments_bwd(c, d, k, n=n, groups=G, fill=True)))
        else:
            open_cap = ops.raster_segments(c, torch.zeros(*c.shape, 11, device=DEV), n=n, groups=G)[0].shape[1]
            assert torch.equal(_bits(one), _bits(ops.raster_segments_bwd(c, d[:, :open_cap].contiguous(), k, n=n, groups=G)))


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _e2e_on_device():
    commands, args, modes, paint, background = e2e_layers()
    N = commands.shape[0] // E2E_G
    return (commands, args, modes, paint, background, commands.to(DEV).view(N, E2E_G, -1), args.to(DEV).view(N, E2E_G, -1, 11),
            modes.to(DEV), paint.to(DEV))


def test_gradient_of_the_fixture_matches_float64_from_the_arguments(gpu_device):
    commands, args, modes, paint, background, c, a, m, p = _e2e_on_device()
    dout = torch.randn(2, 3, E2E_SIZE, E2E_SIZE, generator=torch.Generator().manual_seed(2)).clamp(-4, 4)
    kw = dict(background=background, size=E2E_SIZE, n=E2E_N, groups=E2E_G)
    _, state = LG.picture64(commands, args.double(), modes.tolist(), paint.double(), **kw)
    want_args, want_paint = LG.picture_backward64(commands, state, paint.double(), dout.double(), background=background, n=E2E_N,
                                                  groups=E2E_G)
    a = a.clone().requires_grad_(True)
    colors, opacity = p[..., :3].clone().requires_grad_(True), p[..., 3].clone().requires_grad_(True)
    img = render.draw_with_grad(c, a, filling=m, colors=colors, opacity=opacity, background=background, size=E2E_SIZE, n=E2E_N)
    img.backward(dout.to(DEV))
    _, (_, _, _, cov, _) = ops.draw_fwd_nn(c.view(-1, 6), a.detach().view(-1, 6, 11), m, p, **kw)
    live, live64 = (cov > 0) & (cov < 1), (state[1] > 0) & (state[1] < 1)
    assert torch.equal(live.cpu(), live64), "the fixture's margins should make the live pixels the same"
    scale = dout.abs().max().item()
    err = (a.grad.cpu().view(-1, 6, 11).double() - want_args).abs().max().item() / scale
    got_paint = torch.cat([colors.grad, opacity.grad.unsqueeze(-1)], -1).cpu()
    err_paint = (got_paint.double() - want_paint).abs().max().item() / (scale * E2E_SIZE ** 2)
    print(f"d / d args of the layered fixture, kernels against float64 with its own arg-min: max err {err:.3e} of max |dout| (bound "
          f"{4 * SPREAD:.1e}), max |gradient| {want_args.abs().max().item():.3e}, {int(live64.sum())} live pixels; d / d colours and "
          f"opacities max err {err_paint:.3e} of max |dout| x pixels (bound {4 * PAINT_SPREAD:.1e}), max {want_paint.abs().max().item():.3e}")
    assert bool(want_args.any()) and bool(want_paint.any())
    assert err <= 4 * SPREAD and err_paint <= 4 * PAINT_SPREAD


@pytest.mark.parametrize("compound", [False, True])
def test_picture_loss_backward_is_the_composition_of_the_four_ops(gpu_device, compound):
    commands, args, modes, paint, background, c, a, m, p = _e2e_on_device()
    a = a.clone().requires_grad_(True)
    colors, opacity = p[0, :, :3].clone().requires_grad_(True), p[..., 3].clone().requires_grad_(True)
    target = torch.rand(2, 3, 33, 33, generator=torch.Generator().manual_seed(1)).to(DEV)
    how = dict(compound=True, fill=True, fill_rule="evenodd") if compound else dict(filling=m)
    res = render.picture_loss(c, a, target, colors=colors, opacity=opacity, background=background, n=E2E_N, **how)
    res["loss"].backward()
    flat_c, flat_a = c.reshape(-1, 6), a.detach().reshape(-1, 6, 11)
    full = torch.cat([colors.detach().expand(2, E2E_G, 3), opacity.detach().unsqueeze(-1)], -1).contiguous()
    mode, tables = ("fill", None) if compound else (None, m)
    if compound:
        segs, counts = ops.raster_segments(flat_c, flat_a, n=E2E_N, groups=E2E_G, fill=True)
        first = None
    else:
        segs, counts, first = ops.raster_segments_layers(flat_c, flat_a, m, n=E2E_N, groups=E2E_G)
    out, cov, idx = ops.raster_sweep_layers_nn(segs, counts, first, tables, full, background=background, size=33, evenodd=compound,
                                               compound=mode)
    img = out.clone().requires_grad_(True)
    (img - target).pow(2).flatten(1).mean(1).mean().backward()
    dcov, dpaint = ops.raster_blend_bwd(cov, counts, first, tables, full, img.grad.contiguous(), segs.shape[1], background=background,
                                        compound=mode)
    dsegs = ops.raster_sweep_layers_bwd(segs, counts, first, tables, cov, idx, dcov, compound=mode)
    want = (ops.raster_segments_bwd(flat_c, dsegs, counts, n=E2E_N, groups=E2E_G, fill=True) if compound
            else ops.raster_segments_layers_bwd(flat_c, dsegs, counts, m, n=E2E_N, groups=E2E_G))
    diff = (a.grad.reshape(-1, 6, 11) - want).abs().max().item()
    print(f"picture_loss backward against the four ops by hand, compound={compound}: max |difference| {diff:.3e}, max |gradient| "
          f"{want.abs().max().item():.3e}")
    assert torch.equal(_bits(a.grad.reshape(-1, 6, 11)), _bits(want)) and bool(want.any())
    assert torch.equal(_bits(opacity.grad), _bits(dpaint[..., 3])) and bool(opacity.grad[:, 0].any())
    assert torch.equal(_bits(colors.grad), _bits(dpaint[..., :3].sum(0))) and bool(colors.grad[0].any())
    assert torch.equal(res["per_icon"], (out - target).pow(2).flatten(1).mean(1))
    pic = render.draw(c, a.detach(), colors=colors.detach(), opacity=opacity.detach(), background=background, size=33, n=E2E_N, **how)
    assert torch.equal(_bits(pic), _bits(out)), "draw_with_grad's picture is not draw's"


# ---- the capability ---------------------------------------------------------------------------------------------------------------
def test_refine_to_pictures_moves_the_hole_of_a_ring_on_the_device(gpu_device):
    commands, target_args, start = shifted_ring()
    filling = torch.tensor([[1, 2]])
    saved = LG.install()
    try:
        target = render.draw(commands, target_args, filling=filling, size=16)
        _, host_history = render.refine_to_pictures(commands, start, target, steps=30, lr=0.1, filling=filling)
    finally:
        LG.restore(saved)
    c, f = commands.to(DEV), filling.to(DEV)
    t = render.draw(c, target_args.to(DEV), filling=f, size=16)
    refined, history = render.refine_to_pictures(c, start.to(DEV), t, steps=30, lr=0.1, filling=f)
    end = render.picture_loss(c, refined, t, filling=f)["loss"].item()
    host_end = host_history[-1].item()
    inner = lambda x: (x.cpu()[0, 1, :5, 9:11] - target_args[0, 1, :5, 9:11]).abs().mean().item()
    # next to it: the one-channel loss in fill mode on the same input.  It paints the hole over (the union of the two
    # squares is the outer one), so all it sees of the inner square is the hairline of its outline
    a = start.to(DEV).clone().requires_grad_(True)
    render.image_loss(c, a, 1 - t[:, 0], fill=True)["loss"].backward()
    b = start.to(DEV).clone().requires_grad_(True)
    render.picture_loss(c, b, t, filling=f)["loss"].backward()
    print(f"refine_to_pictures, 30 steps at 16 x 16 on the ring with its hole moved by 1.5: loss {history[0].item():.3e} -> "
          f"{history[-1].item():.3e} (after the last step {end:.3e}); the restatement's loop {host_history[0].item():.3e} -> "
          f"{host_end:.3e}; inner vertices {inner(start):.3f} -> {inner(refined):.3f} from the target's.  Gradient on the inner "
          f"square's arguments: picture_loss max {b.grad[0, 1].abs().max().item():.3e}, image_loss(fill=True) max "
          f"{a.grad[0, 1].abs().max().item():.3e}")
    assert history.is_cuda and history.shape == (30,) and history[-1].item() < history[0].item()
    assert inner(refined) < inner(start), "the inner vertices did not move towards the target's"
    assert history[-1].item() <= 1.25 * host_end
    assert torch.equal(refined[..., :5], start.to(DEV)[..., :5]) and bool(b.grad[0, 1].any())


# ---- memory -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compound", [False, True])
def test_nothing_uninitialised_is_read_forward_or_backward(gpu_device, forwards, compound):
    f = forwards("gaps_s33")
    kw = f["kw"]
    c, a = f["c"].view(-1, kw["groups"], 6), f["a"].view(-1, kw["groups"], 6, 11)
    how = dict(compound=True, fill=True, fill_rule="evenodd") if compound else dict(filling=f["modes"])
    dout = blend_dout("poison", (c.shape[0], 3, 33, 33)).to(DEV)

    def run():
        args = a.clone().requires_grad_(True)
        colors, opacity = f["paint"][..., :3].clone().requires_grad_(True), f["paint"][..., 3].clone().requires_grad_(True)
        img = render.draw_with_grad(c, args, colors=colors, opacity=opacity, background=f["background"], size=33, n=4, **how)
        img.backward(dout)
        torch.cuda.synchronize()
        return img.detach(), args.grad, colors.grad, opacity.grad

    runs = three_runs(run)
    assert all(bool(torch.isfinite(t).all()) for t in runs[0]) and bool(runs[0][1].any()) and bool(runs[0][2].any())
    for tag, other in zip(("NaN", "zero"), runs[1:]):
        for what, x, y in zip(("picture", "d args", "d colors", "d opacity"), runs[0], other):
            assert torch.equal(_bits(x), _bits(y)), f"{what} differs under {tag} poison"


def test_forward_and_backward_allocate_their_results_only(gpu_device):
    """16 icons of 8 x 32 tokens at 64 x 64: draw's budget (workspace, tables, picture) plus cov, idx, dcov, dsegs, dargs, dpaint"""
    from tests.test_metrics_gpu import _random_sequences
    commands, args = _random_sequences(16, 8, 32, seed=6)
    c, a = commands.reshape(128, 32).float().to(DEV), args.reshape(128, 32, 11).float().to(DEV)
    modes = torch.randint(0, 3, (16, 8), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    paint = torch.cat([render.palette(8, device=DEV).expand(16, 8, 3), torch.full((16, 8, 1), 0.75, device=DEV)], -1).contiguous()
    dout = torch.ones(16, 3, 64, 64, device=DEV)

    def run():
        out, saved = ops.draw_fwd_nn(c, a, modes, paint, size=64, n=10, groups=8)
        return (out, saved) + ops.draw_bwd(c, modes, paint, saved, dout, n=10, groups=8)

    run()                                                    # (code objects loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out, saved, dargs, dpaint = run()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    segs, counts, first, cov, idx = saved
    draw = lib.load().dsvg_raster_workspace_bytes(16, 8, 32, 10, 1) + out.numel() * 4 + first.numel() * 4 + counts.numel() * 4
    budget = draw + (cov.numel() * 2 + idx.numel() + segs.shape[0] * segs.shape[1] * 4 + dargs.numel() + dpaint.numel()) * 4
    print(f"forward twin + backward: peak allocation grew by {grown} bytes; draw's {draw} + cov + idx + dcov + dsegs + dargs + dpaint "
          f"= {budget}")
    assert grown <= budget + (64 << 10) and bool(torch.isfinite(dargs).all()) and bool(dargs.any()) and bool(dpaint.any())


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(gpu_device, forwards):
    f = forwards("g3_s33")
    c, a = f["c"].view(-1, 3, 6), f["a"].view(-1, 3, 6, 11)
    with pytest.raises(ValueError, match="float32 args"):
        render.draw_with_grad(c, a.long(), filling=f["modes"])
    with pytest.raises(ValueError, match="target_pictures"):
        render.picture_loss(c, a, f["out"][:, 0], filling=f["modes"])
    segs, counts, first, modes, paint, cov, idx = (f[k] for k in ("segs", "counts", "first", "modes", "paint", "cov", "idx"))
    cap, dout = segs.shape[1], torch.zeros_like(f["out"])
    dcov, _ = ops.raster_blend_bwd(cov, counts, first, modes, paint, dout, cap, background=f["background"])
    with pytest.raises(lib.DsvgError, match="pixels per side"):
        ops.raster_sweep_layers_nn(segs, counts, first, modes, paint, size=0)
    with pytest.raises(lib.DsvgError, match="background"):
        ops.raster_sweep_layers_nn(segs, counts, first, modes, paint, background=(0.0, 1.5, 0.0))
    with pytest.raises(AssertionError, match="modes"):
        ops.raster_sweep_layers_nn(segs, counts, first, modes[:, :2].contiguous(), paint)
    with pytest.raises(AssertionError, match="layer_first"):
        ops.raster_blend_bwd(cov, counts, first[:, :3].contiguous(), modes, paint, dout, cap)
    with pytest.raises(AssertionError, match="paint"):
        ops.raster_blend_bwd(cov, counts, first, modes, paint[..., :3].contiguous(), dout, cap)
    with pytest.raises(AssertionError, match="dout"):
        ops.raster_blend_bwd(cov, counts, first, modes, paint, dout[:, :2].contiguous(), cap)
    with pytest.raises(AssertionError, match="cov|layer_first"):
        ops.raster_sweep_layers_bwd(segs, counts, first, modes, cov[:, :2].contiguous(), idx, dcov)
    with pytest.raises(AssertionError):
        ops.raster_sweep_layers_bwd(segs, counts, first, modes, cov, idx.long(), dcov)
    with pytest.raises(lib.DsvgError, match="stroke_width"):
        ops.raster_sweep_layers_bwd(segs, counts, first, modes, cov, idx, dcov, stroke_width=-1.0)
    dsegs = ops.raster_sweep_layers_bwd(segs, counts, first, modes, cov, idx, dcov)
    with pytest.raises(AssertionError, match="modes"):
        ops.raster_segments_layers_bwd(f["c"], dsegs, counts, modes[:, :2].contiguous(), n=4, groups=3)
    with pytest.raises((lib.DsvgError, AssertionError), match="2..64|dsegs"):
        ops.raster_segments_layers_bwd(f["c"], dsegs, counts, modes, n=65, groups=3)
    with pytest.raises(lib.DsvgError):
        ops.raster_blend_bwd(cov.cpu(), counts.cpu(), first.cpu(), modes.cpu(), paint.cpu(), dout.cpu(), cap)
    L = lib.load()
    B, G = segs.shape[0], 3
    white = (lib.C.c_float * 3)(1.0, 1.0, 1.0)
    bg = lib.C.cast(white, lib.C.c_void_p)
    p = (segs.data_ptr(), counts.data_ptr(), first.data_ptr(), modes.data_ptr(), paint.data_ptr())
    assert L.dsvg_raster_sweep_layers_nn(*p, bg, B, cap, G, 33, 3.2, 0, f["out"].data_ptr(), cov.data_ptr(), None, None) != 0
    assert b"null pointer" in L.dsvg_last_error()
    assert L.dsvg_raster_blend_bwd(cov.data_ptr(), counts.data_ptr(), None, modes.data_ptr(), paint.data_ptr(), bg, dout.data_ptr(), B,
                                   cap, G, 33, 0, dcov.data_ptr(), dsegs.data_ptr(), None) != 0
    assert b"null pointer" in L.dsvg_last_error()
    assert L.dsvg_raster_blend_bwd(cov.data_ptr(), counts.data_ptr(), first.data_ptr(), modes.data_ptr(), paint.data_ptr(), bg,
                                   dout.data_ptr(), B, cap, G, 0, 0, dcov.data_ptr(), dsegs.data_ptr(), None) != 0
    assert b"pixels per side" in L.dsvg_last_error()
    assert L.dsvg_raster_sweep_layers_bwd(*p[:4], cov.data_ptr(), idx.data_ptr(), None, B, cap, G, 33, 3.2, 0, dsegs.data_ptr(),
                                          None) != 0 and b"null pointer" in L.dsvg_last_error()
    assert L.dsvg_raster_sweep_layers_bwd(*p[:4], cov.data_ptr(), idx.data_ptr(), dcov.data_ptr(), B, cap, G, 33, 3.2, 1, dsegs.data_ptr(),
                                          None) != 0 and b"unknown flags" in L.dsvg_last_error()
    assert L.dsvg_raster_segments_layers_bwd(f["c"].data_ptr(), dsegs.data_ptr(), counts.data_ptr(), None, B, G, 6, 4, dsegs.data_ptr(),
                                             None) != 0 and b"null pointer" in L.dsvg_last_error()
