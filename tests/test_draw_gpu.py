"""deepsvg_amd.render.draw on a real MI355X: dsvg_raster_segments_layers and dsvg_raster_sweep_layers (csrc/raster.hip) against
the existing rasteriser bit for bit where the two must agree, against the float64 restatement of
tests/raster_layers_ref.py everywhere else, and their exactness properties.  Every test prints the largest error it saw
before it asserts.

Tolerances (derived in tests/test_draw_host.py and tests/test_render_host.py): chord vertices POINT_ATOL; a pixel and channel
of an icon with K layers that have chords K * ink_atol(size) + K * 2**-22.  No pixel is excluded."""
import pytest
import torch

from deepsvg_amd import lib, ops, render
from tests import helpers as H
from tests import raster_layers_ref as LR
from tests import raster_ref as RR
from tests.poison import three_runs
from tests.test_draw_host import (BLUE, RED, _check_ring, _check_two_colours, layered_atol, random_paint, ring, ring_masks,
                                   two_squares)
from tests.test_metrics_gpu import _random_sequences
from tests.test_render_gpu import LDS_CHORDS, _flat
from tests.test_render_host import POINT_ATOL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- bit equality with the existing rasteriser ------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("size", [8, 64, 100])
def test_one_group_black_on_white_is_one_minus_rasterize(gpu_device, size, fill):
    """fmaf(cov, 0 - 1, 1) is the correctly rounded 1 - cov"""
    for dtype, L in ((torch.int64, 32), (torch.float32, 66)):
        commands, args = _random_sequences(3, 1, L, seed=300 + L)
        c, a = _flat(commands, args, dtype)
        want = 1 - render.rasterize(c, a, size=size, fill=fill)
        assert 0.0 < want.mean().item() < 1.0
        got = render.draw(c, a, size=size, fill=fill)                                   # [N, S]: G = 1
        assert got.shape == (3, 3, size, size) and got.dtype == torch.float32
        filling = torch.full((3, 1, 1), 1 if fill else 0, device=DEV)
        as_groups = render.draw(c.view(3, 1, L), a.view(3, 1, L, 11), filling=filling, size=size)
        for ch in range(3):
            diff = (got[:, ch] - want).abs().max().item()
            print(f"draw[:, {ch}] against 1 - rasterize, size={size} fill={fill} {dtype}: max difference {diff:.3e}")
            assert torch.equal(_bits(got[:, ch]), _bits(want)) and torch.equal(_bits(as_groups[:, ch]), _bits(want))


# ---- segments ---------------------------------------------------------------------------------------------------------------
def _icons(B, G, L, seed):
    """commands from all seven ids (l and c half of the time) and arguments from -1..255 in every slot, as
    tests/test_metrics_gpu.py::_random_sequences; with G >= 3 the last group of icon 0 and the first group of icon B - 1 are
    empty, with G >= 4 also group G // 2 of every icon"""
    gen = torch.Generator().manual_seed(seed)
    pool = torch.tensor([0, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6])
    commands = pool[torch.randint(0, len(pool), (B, G, L), generator=gen)]
    if G >= 3:
        commands[0, G - 1] = 4
        commands[B - 1, 0] = 4
    if G >= 4:
        commands[:, G // 2] = 4
    return commands, torch.randint(-1, 256, (B, G, L, 11), generator=gen)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [2, 10])
def test_uniform_mode_tables_give_the_records_of_raster_segments(gpu_device, n, dtype):
    for G, L in ((1, 32), (8, 33)):
        commands, args = _icons(3, G, L, seed=50 + n)
        commands[1, 0, 1], commands[1, 0, 2] = 1, 2                # (every icon has chords)
        c, a = _flat(commands, args, dtype)
        for mode, fill in ((0, False), (1, True), (2, True), (5, False)):
            modes = torch.full((3, G), mode, dtype=torch.int32, device=DEV)
            segs, counts, first = ops.raster_segments_layers(c, a, modes, n=n, groups=G)
            want, want_counts = ops.raster_segments(c, a, n=n, groups=G, fill=fill)
            assert segs.shape == (3, G * (L * (n - 1) + (L + 1) // 2), 5) and torch.equal(counts, want_counts)
            live = torch.arange(want.shape[1], device=DEV).view(1, -1, 1) < counts.view(-1, 1, 1)
            assert int(counts.min()) > 0
            assert torch.equal(_bits(segs[:, :want.shape[1]]) * live, _bits(want) * live), (G, mode)
            assert torch.equal(first[:, -1], counts) and bool((first[:, 0] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [2, 7, 10])
def test_mixed_mode_segments_match_the_restatement(gpu_device, n, dtype):
    worst = 0.0
    for B, G, L in ((3, 8, 12), (2, 3, 66), (1, 8, 256)):
        commands, args = _icons(B, G, L, seed=70 + n + L)
        modes = torch.randint(0, 3, (B, G), generator=torch.Generator().manual_seed(n + L), dtype=torch.int32)
        c, a = _flat(commands, args, dtype)
        segs, counts, first = ops.raster_segments_layers(c, a, modes.to(DEV), n=n, groups=G)
        per_image = LR.group_chords(c.cpu(), a.cpu(), modes.tolist(), n, G)
        segs = segs.cpu()
        for i, layers in enumerate(per_image):
            chords, want_first = LR.image_chords(layers)
            assert first.dtype == torch.int32 and first[i].tolist() == want_first, "layer_first differs"
            k = want_first[-1]
            assert int(counts[i]) == k and k > 0
            got, flags = segs[i, :k, :4], _bits(segs[i, :k, 4])
            assert torch.equal(flags, RR.records(chords)[1]), "flag words differ"
            assert not bool(torch.isnan(got).any())
            worst = max(worst, (got[:, :2].double() - chords["a"]).abs().max().item(),
                        (got[:, :2].double() + got[:, 2:].double() - chords["b"]).abs().max().item())
        empty = first[:, 1:] == first[:, :-1]
        assert bool(empty[0, G - 1]) and bool(empty[B - 1, 0]) and (G < 4 or bool(empty[:, G // 2].all()))
    print(f"raster_segments_layers vs float64 restatement n={n} {dtype}: vertices {worst:.3e} (bound {POINT_ATOL:.1e})")
    assert worst <= POINT_ATOL


# ---- the sweep against the restatement --------------------------------------------------------------------------------------
SHAPES = {
    "sub_quadrant": dict(N=3, G=3, L=8, n=2, size=8, dtype=torch.int64),            # less than one quadrant
    "ends_in_tile": dict(N=2, G=8, L=32, n=10, size=64, dtype=torch.float32),       # layer ends inside a 512-chord tile
    "spans_tiles": dict(N=2, G=2, L=64, n=10, size=100, dtype=torch.int64),         # a layer over several tiles, size % 32 != 0
    "token_limit": dict(N=1, G=32, L=64, n=10, size=32, dtype=torch.float32),       # G * L = 2048
}
RULES = [(None, False), (None, True), ("fill", False), ("fill", True), ("stroke", False)]


def _case(shape):
    s = SHAPES[shape]
    commands, args = _icons(s["N"], s["G"], s["L"], seed=len(shape))
    if shape == "spans_tiles":            # 60 drawing rows of 64 in four sub-paths: 540 chords and more per layer
        commands[(commands != 1) & (commands != 2)] = 2
        commands[..., ::16] = 0
    modes, paint, background = random_paint(s["N"], s["G"], seed=s["L"])
    return s, _flat(commands, args, s["dtype"]), modes, paint, background


@pytest.fixture(scope="module")
def oracle():
    """the float64 pictures, computed once per (shape, compound, evenodd) and left unchanged; with them the number of
    layers that have chords, per icon"""
    cache = {}

    def get(shape, compound, evenodd):
        if (shape, compound, evenodd) not in cache:
            s, (c, a), modes, paint, background = _case(shape)
            want = LR.draw(c.cpu(), a.cpu(), None if compound else modes, paint, background=background, size=s["size"],
                           evenodd=evenodd, compound=compound, n=s["n"], groups=s["G"], as_double=True)
            if compound:
                layers = [1] * s["N"]
            else:
                layers = [sum(1 for ly in icon if ly["a"].shape[0])
                          for icon in LR.group_chords(c.cpu(), a.cpu(), modes.tolist(), s["n"], s["G"])]
            cache[shape, compound, evenodd] = want, layers
        return cache[shape, compound, evenodd]
    return get


@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("compound,evenodd", RULES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sweep_matches_the_restatement(gpu_device, oracle, shape, compound, evenodd, cull):
    s, (c, a), modes, paint, background = _case(shape)
    want, layers = oracle(shape, compound, evenodd)
    got = ops.draw(c, a, None if compound else modes.to(DEV), paint.to(DEV), background=background, size=s["size"],
                   evenodd=evenodd, compound=compound, n=s["n"], groups=s["G"], cull=cull).cpu()
    assert got.shape == want.shape == (s["N"], 3, s["size"], s["size"]) and got.dtype == torch.float32
    assert max(layers) >= (1 if compound else 2)
    if shape == "spans_tiles" and not compound:
        first = ops.raster_segments_layers(c, a, modes.to(DEV), n=s["n"], groups=s["G"])[2]
        assert int((first[:, 1:] - first[:, :-1]).max()) > LDS_CHORDS
    for i, k in enumerate(layers):
        err = (got[i].double() - want[i]).abs().max().item()
        print(f"draw {shape} icon {i} compound={compound} evenodd={evenodd} cull={cull}: {k} layers, max err {err:.3e} "
              f"(bound {layered_atol(s['size'], k):.3e}), mean {got[i].mean().item():.4f}")
        assert err <= layered_atol(s["size"], k)
    assert 0.0 < got.mean().item() < 1.0 and got.min().item() >= 0.0 and got.max().item() <= 1.0
    assert (got - torch.tensor(background).view(1, 3, 1, 1)).abs().max().item() > 0.1, "an empty picture"


def test_a_layer_table_of_2048_groups_fits(gpu_device):
    """G = 2048, L = 1: the largest layer table next to the chord tiles; every group draws one line from (0, 0)"""
    gen = torch.Generator().manual_seed(2048)
    commands = torch.ones(1, 2048, 1)
    args = torch.randint(0, 256, (1, 2048, 1, 11), generator=gen).float()
    modes, paint, background = random_paint(1, 2048, seed=11)
    modes[modes == 2] = 0
    paint[..., 3] *= 0.05
    for cull in (False, True):
        got = ops.draw(*_flat(commands, args, torch.float32), modes.to(DEV), paint.to(DEV), background=background, size=32, n=2,
                       groups=2048, cull=cull).cpu()
        want = LR.draw(commands.view(2048, 1), args.view(2048, 1, 11), modes, paint, background=background, size=32, n=2,
                       groups=2048, as_double=True)
        err = (got.double() - want).abs().max().item()
        print(f"2048 layers, cull={cull}: max err {err:.3e} (bound {layered_atol(32, 2048):.3e})")
        assert err <= layered_atol(32, 2048) and 0.0 < got.mean().item() < 1.0


# ---- closed forms -----------------------------------------------------------------------------------------------------------
def test_analytic_ring_and_two_colours_on_the_device(gpu_device):
    commands, args = (t.to(DEV) for t in ring())
    layered = render.draw(commands, args, filling=torch.tensor([[1, 2]], device=DEV), size=64)
    _check_ring(layered[0].cpu())
    # the same ring as one compound path: the same bits off the outlines; on them d is a few fp32 roundings instead of 0 and
    # 0.5 + d / s on one side of 0.5 need not round as 1 - (0.5 - d / s) does on the other
    evenodd = render.draw(commands, args, compound=True, fill=True, fill_rule="evenodd", size=64)
    _check_ring(evenodd[0].cpu())
    edge = ring_masks()[2].to(DEV)
    diff = (evenodd - layered).abs().max().item()
    print(f"compound even-odd ring against fill + erase: max difference {diff:.3e}, all of it on the outlines")
    assert torch.equal(_bits(evenodd[0][:, ~edge]), _bits(layered[0][:, ~edge])) and diff <= layered_atol(64, 2)
    disc = render.draw(commands, args, compound=True, fill=True, size=64)[0]
    assert disc[0, 16, 16] == 0.0 and layered[0, 0, 16, 16] == 1.0
    gone = render.draw(commands.flip(1), args.flip(1), filling=torch.tensor([[2, 1]], device=DEV), size=64)[0]
    assert gone[0, 16, 16] == 0.0
    commands, args = (t.to(DEV) for t in two_squares())
    colors = torch.tensor([RED, BLUE], device=DEV)
    _check_two_colours(render.draw(commands, args, fill=True, colors=colors, opacity=0.5, size=64)[0].cpu())
    wild = torch.tensor([[7.0, float("nan"), -3.0], [0.0, 0.0, 1.0]], device=DEV)
    _check_two_colours(render.draw(commands, args, fill=True, colors=wild, opacity=torch.tensor([0.5, 0.5]), size=64)[0].cpu())


# ---- reproducibility --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["ends_in_tile", "spans_tiles"])
def test_culling_and_a_second_run_leave_every_bit_as_it_is(gpu_device, shape):
    s, (c, a), modes, paint, background = _case(shape)
    for compound, evenodd in RULES:
        for width in (3.2, 0.0, 40.0):
            kw = dict(background=background, size=s["size"], stroke_width=width, evenodd=evenodd, compound=compound, n=s["n"],
                      groups=s["G"])
            tables = (None if compound else modes.to(DEV), paint.to(DEV))
            plain = ops.draw(c, a, *tables, cull=False, **kw)
            culled = ops.draw(c, a, *tables, cull=True, **kw)
            again = ops.draw(c, a, *tables, cull=False, **kw)
            diff = (plain - culled).abs().max().item()
            print(f"{shape} compound={compound} evenodd={evenodd} width={width}: max |cull=0 - cull=1| {diff:.3e}")
            assert torch.equal(_bits(plain), _bits(culled)), "culling changed the picture"
            assert torch.equal(_bits(plain), _bits(again)), "two runs differ in bits"


# ---- no dependence on memory nobody wrote -----------------------------------------------------------------------------------
def test_records_past_the_count_and_tables_of_empty_groups_are_not_used(gpu_device):
    s, (c, a), modes, paint, background = _case("ends_in_tile")
    modes, paint = modes.to(DEV), paint.to(DEV)
    segs, counts, first = ops.raster_segments_layers(c, a, modes, n=s["n"], groups=s["G"])
    kw = dict(background=background, size=s["size"])
    want = ops.raster_sweep_layers(segs, counts, first, modes, paint, **kw)
    dead = torch.arange(segs.shape[1], device=DEV).view(1, -1, 1) >= counts.view(-1, 1, 1)
    assert bool(dead.any(1).all())
    empty = first[:, 1:] == first[:, :-1]
    assert bool(empty.any(1).all()) and not bool(empty.all(1).any())
    for poison in (float("nan"), 3e38):
        dirty = torch.where(dead, torch.full_like(segs, poison), segs)
        got = ops.raster_sweep_layers(dirty, counts, first, modes, paint, **kw)
        assert torch.equal(_bits(got), _bits(want)), f"records past the count were read ({poison})"
        # the paint and the mode of a group without chords; of layer_first the sweep uses entries 1..G - 1 (where one layer
        # ends the next starts; the first starts at 0 and the last ends at the count), clamped into 0..count: the two others
        # may hold anything
        dirty_paint = torch.where(empty.unsqueeze(-1), torch.full_like(paint, poison), paint)
        dirty_modes = torch.where(empty, 2 - modes.clamp(0, 2), modes)
        dirty_first = first.clone()
        dirty_first[:, 0], dirty_first[:, -1] = -12345, 2 ** 30
        got = ops.raster_sweep_layers(segs, counts, dirty_first, dirty_modes, dirty_paint, **kw)
        assert torch.equal(_bits(got), _bits(want)), f"the tables of empty groups were used ({poison})"


@pytest.mark.parametrize("compound", [False, True])
def test_every_element_is_written_and_nothing_uninitialised_is_read(gpu_device, compound):
    s, (c, a), modes, paint, _ = _case("ends_in_tile")
    G, L = s["G"], s["L"]
    c, a = c.view(s["N"], G, L), a.view(s["N"], G, L, 11)
    kw = dict(compound=True, fill=True, fill_rule="evenodd") if compound else dict(filling=modes.to(DEV))

    def run():
        out = render.draw(c, a, colors=paint[..., :3].to(DEV), opacity=paint[..., 3].to(DEV), size=100, **kw)
        torch.cuda.synchronize()
        return out

    runs = three_runs(run)
    assert bool(torch.isfinite(runs[0]).all()) and 0.0 < runs[0].mean().item() < 1.0
    for tag, other in zip(("NaN", "zero"), runs[1:]):
        assert torch.equal(_bits(other), _bits(runs[0])), f"the picture differs under {tag} poison"


def test_draw_allocates_the_workspace_the_tables_and_the_output_only(gpu_device):
    """16 icons of 8 x 32 tokens at 64 x 64: a [pixels, chords] matrix would be hundreds of MB, a copy of the inputs 393 KB"""
    commands, args = _random_sequences(16, 8, 32, seed=6)
    c, a = commands.to(DEV), args.to(DEV)
    filling = torch.randint(0, 3, (16, 8, 1), generator=torch.Generator().manual_seed(1)).to(DEV)
    colors = render.palette(8, device=DEV)
    render.draw(c, a, filling=filling, colors=colors, size=64)                   # (code objects loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = render.draw(c, a, filling=filling, colors=colors, size=64)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    tables = 16 * 8 * (4 + 16) + 16 * 9 * 4 + 16 * 4          # modes, paint, layer_first, seg_counts
    budget = lib.load().dsvg_raster_workspace_bytes(16, 8, 32, 10, 1) + out.numel() * 4 + tables
    print(f"draw: peak allocation grew by {grown} bytes, workspace + tables + output {budget}")
    assert grown <= budget + (64 << 10) and bool(torch.isfinite(out).all())


def test_bad_arguments_are_refused(gpu_device):
    s, (c, a), modes, paint, background = _case("sub_quadrant")
    modes, paint = modes.to(DEV), paint.to(DEV)
    segs, counts, first = ops.raster_segments_layers(c, a, modes, n=2, groups=3)
    with pytest.raises(lib.DsvgError, match="pixels per side"):
        ops.raster_sweep_layers(segs, counts, first, modes, paint, size=0)
    with pytest.raises(lib.DsvgError, match="background"):
        ops.raster_sweep_layers(segs, counts, first, modes, paint, background=(0.0, 1.5, 0.0))
    with pytest.raises(lib.DsvgError, match="2..64"):
        ops.raster_segments_layers(c, a, modes, n=65, groups=3)
    with pytest.raises(AssertionError):
        ops.raster_segments_layers(c, a, modes[:, :2], n=2, groups=3)
    with pytest.raises(AssertionError):
        ops.raster_sweep_layers(segs, counts, first, modes.long(), paint)
    L = lib.load()
    assert L.dsvg_raster_sweep_layers(segs.data_ptr(), counts.data_ptr(), None, None, paint.data_ptr(), None, 3, segs.shape[1], 3,
                                      8, 3.2, 0, None, None) != 0
    assert b"null pointer" in L.dsvg_last_error()


# ---- with the data set ------------------------------------------------------------------------------------------------------
def test_a_data_set_batch_is_drawn_with_its_filling(gpu_device):
    from tests.test_dataset import _dataset
    icons, fillings, (G, S, T), _ = H.golden_batch("icons")
    keys = ["commands", "args", "filling"]
    ds = _dataset([[g] for g in icons], fillings, G, S, T, keys, gpu_device)
    idx = list(range(min(len(icons), 12)))
    batch = ds.batch(idx, random_aug=False)
    N = len(idx)
    assert batch["commands"].shape == (N, G, S + 2) and batch["filling"].shape == (N, G, 1) and batch["filling"].is_cuda
    assert batch["filling"].flatten(1).tolist() == [fillings[i] + [0] * (G - len(fillings[i])) for i in idx]
    colors = render.palette(G, device=DEV)
    got = render.draw(batch["commands"], batch["args"], filling=batch["filling"], colors=colors, size=64).cpu()
    c, a = batch["commands"].reshape(N * G, S + 2).cpu(), batch["args"].reshape(N * G, S + 2, 11).cpu()
    modes = batch["filling"].reshape(N, G).cpu()
    paint = torch.cat([colors.cpu().expand(N, G, 3), torch.ones(N, G, 1)], -1)
    want = LR.draw(c, a, modes, paint, size=64, groups=G, as_double=True)
    layers = [sum(1 for ly in icon if ly["a"].shape[0]) for icon in LR.group_chords(c, a, modes.tolist(), 10, G)]
    for i, k in enumerate(layers):
        err = (got[i].double() - want[i]).abs().max().item()
        print(f"data-set icon {i}: filling {modes[i].tolist()}, {k} layers, max err {err:.3e} (bound {layered_atol(64, k):.3e})")
        assert err <= layered_atol(64, k)
    assert max(layers) >= 2 and bool((modes > 0).any()), "the golden icons changed: nothing layered is drawn"
    assert 0.0 < got.mean().item() < 1.0
