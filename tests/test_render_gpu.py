"""deepsvg_amd.render on a real MI355X: dsvg_raster_segments and dsvg_raster_sweep (csrc/raster.hip) against the float64
restatement of tests/raster_ref.py, their exactness properties, and reconstruction_images / interpolate end to end.  Every
test prints the largest error it saw before it asserts.

Tolerances (derived in tests/test_render_host.py): chord vertices POINT_ATOL = 5e-4, the start vertex as the record holds it
and the end vertex read back as a + (b - a); ink 2 * DIST_ATOL / s with DIST_ATOL = 1e-3 and s = 256 / size.  No pixel is
excluded."""
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import lib, ops, render
from tests import helpers as H
from tests import raster_ref as RR
from tests.test_metrics_gpu import _random_sequences
from tests.test_render_host import POINT_ATOL, ink_atol, square, square_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
LDS_CHORDS = 512       # RS_CHORDS of csrc/raster.hip: chords per LDS tile of the sweep


def _as(t, dtype):
    return (t.long() if dtype == torch.int64 else t.float()).to(DEV)


def _flat(commands, args, dtype):
    B, G, L = commands.shape
    return _as(commands.reshape(B * G, L), dtype), _as(args.reshape(B * G, L, 11), dtype)


def _check_segments(c, a, n, G, fill, exact=False):
    """ops.raster_segments against the restatement's chord list -> (max error of the start vertices, of the end vertices)"""
    segs, counts = ops.raster_segments(c, a, n=n, groups=G, fill=fill)
    lists = RR.chord_list(c.cpu(), a.cpu(), n=n, groups=G, fill=fill)
    L = c.shape[1]
    assert segs.shape == (len(lists), max(G * (L * (n - 1) + ((L + 1) // 2 if fill else 0)), 1), 5)
    assert counts.dtype == torch.int32 and counts.tolist() == [len(ch["seq"]) for ch in lists], "chord counts differ"
    segs = segs.cpu()
    worst_a = worst_b = 0.0
    for i, ch in enumerate(lists):
        k = len(ch["seq"])
        if not k:
            continue
        got, flags = segs[i, :k, :4], segs[i, :k, 4].contiguous().view(torch.int32)
        want, want_flags = RR.records(ch)
        assert torch.equal(flags, want_flags), "flag words differ"
        assert not bool(torch.isnan(got).any())
        worst_a = max(worst_a, (got[:, :2].double() - ch["a"]).abs().max().item())
        worst_b = max(worst_b, (got[:, :2].double() + got[:, 2:].double() - ch["b"]).abs().max().item())
        if exact:
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "records differ in bits"
        # a vertex that two chords share is one number: where a command or a closing chord starts, the input itself
        closing = ch["back"] > 0
        first = ~closing & ((torch.cumsum((~closing).long(), 0) - 1) % (n - 1) == 0)
        sel = first | closing
        assert torch.equal(got[sel, :2], ch["a"][sel].float()), "a command does not start at the row before's end position"
    return worst_a, worst_b


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [2, 7, 10, 64])
def test_segments_match_the_restatement(gpu_device, n, dtype, fill):
    worst_a = worst_b = 0.0
    for B in (1, 5):
        for G in (1, 8):
            for L in (1, 32, 66):
                commands, args = _random_sequences(B, G, L, seed=1000 * B + 100 * G + L + n)
                ea, eb = _check_segments(*_flat(commands, args, dtype), n, G, fill)
                worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
    print(f"raster_segments vs float64 restatement n={n} {dtype} fill={fill}: start vertices {worst_a:.3e}, end {worst_b:.3e}")
    assert worst_a <= POINT_ATOL and worst_b <= POINT_ATOL


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [2, 7, 10, 64])
def test_segments_of_lines_with_integer_arguments_are_bit_equal(gpu_device, n, dtype):
    for G, L in ((1, 32), (8, 66)):
        commands, args = _random_sequences(3, G, L, seed=40 + n)
        commands[commands == 2] = 1                       # `l` only
        for fill in (False, True):
            _check_segments(*_flat(commands, args, dtype), n, G, fill, exact=True)


@pytest.mark.parametrize("n", [2, 10])
def test_consecutive_commands_share_vertices_bit_for_bit_with_float_arguments(gpu_device, n):
    commands, _ = _random_sequences(4, 8, 32, seed=9)
    args = torch.rand(4, 8, 32, 11, generator=torch.Generator().manual_seed(10)) * 256.0
    for fill in (False, True):
        ea, eb = _check_segments(*_flat(commands, args, torch.float32), n, 8, fill)
        print(f"float arguments n={n} fill={fill}: start vertices {ea:.3e}, end {eb:.3e}")
        assert ea <= POINT_ATOL and eb <= POINT_ATOL


@pytest.mark.parametrize("G,L", [(8, 256), (1, 2048)])
def test_segments_at_2048_tokens_per_image(gpu_device, G, L):
    commands, args = _random_sequences(2, G, L, seed=77)
    for fill in (False, True):
        ea, eb = _check_segments(*_flat(commands, args, torch.float32), 10, G, fill)
        print(f"raster_segments G={G} L={L} fill={fill}: start vertices {ea:.3e}, end {eb:.3e}")
        assert ea <= POINT_ATOL and eb <= POINT_ATOL


def test_bad_arguments_are_refused(gpu_device):
    c, a = torch.zeros(2, 4, device=DEV), torch.zeros(2, 4, 11, device=DEV)
    with pytest.raises(lib.DsvgError, match="tokens per image"):
        ops.raster_segments(torch.zeros(1, 2049, device=DEV), torch.zeros(1, 2049, 11, device=DEV))
    with pytest.raises(lib.DsvgError, match="tokens per image"):
        ops.raster_segments(torch.zeros(8, 257, device=DEV), torch.zeros(8, 257, 11, device=DEV), groups=8)
    for n in (1, 65):
        with pytest.raises(lib.DsvgError, match="2..64"):
            ops.raster_segments(c, a, n=n)
    with pytest.raises(lib.DsvgError):
        ops.raster_segments(c.cpu(), a.cpu())
    segs, counts = ops.raster_segments(c, a)
    with pytest.raises(lib.DsvgError, match="pixels per side"):
        ops.raster_sweep(segs, counts, size=0)
    with pytest.raises(lib.DsvgError, match="stroke_width"):
        ops.raster_sweep(segs, counts, stroke_width=-1.0)
    L = lib.load()
    assert L.dsvg_raster_workspace_bytes(3, 8, 32, 10, 0) == 3 * 8 * 32 * 9 * 20
    assert L.dsvg_raster_workspace_bytes(3, 8, 32, 10, 1) == 3 * 8 * (32 * 9 + 16) * 20
    assert L.dsvg_raster_segments(0, c.data_ptr(), a.data_ptr(), 2, 1, 4, 10, 0, segs.data_ptr(), 8, counts.data_ptr(), None) != 0
    assert b"buffer" in L.dsvg_last_error()


# ---- the sweep --------------------------------------------------------------------------------------------------------------
def _batches():
    """`long`: more chords in an image than one LDS tile; `gap`: an empty image between two others"""
    commands, args = _random_sequences(2, 8, 66, seed=21)
    gap_c, gap_a = _random_sequences(3, 4, 12, seed=22)
    gap_c[1] = 4
    return {"long": (commands, args, 8), "gap": (gap_c, gap_a, 4)}


@pytest.fixture(scope="module")
def oracle():
    """the float64 images of the two batches, computed once per (batch, size, fill) and left unchanged"""
    batches, images = _batches(), {}

    def get(name, size, fill):
        commands, args, G = batches[name]
        if (name, size, fill) not in images:
            c, a = _flat(commands, args, torch.int64)
            images[name, size, fill] = RR.rasterize(c.cpu(), a.cpu(), size=size, fill=fill, n=10, groups=G, as_double=True)
        return commands, args, G, images[name, size, fill]
    return get


@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("cull", [False, True])
@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("size", [8, 32, 64, 100])
@pytest.mark.parametrize("name", ["long", "gap"])
def test_sweep_matches_the_restatement(gpu_device, oracle, name, size, fill, cull, dtype):
    commands, args, G, want = oracle(name, size, fill)
    c, a = _flat(commands, args, dtype)
    segs, counts = ops.raster_segments(c, a, n=10, groups=G, fill=fill)
    if name == "long":
        assert int(counts.min()) > LDS_CHORDS
    got = ops.raster_sweep(segs, counts, size=size, fill=fill, cull=cull).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    err = (got.double() - want).abs().max().item()
    print(f"raster_sweep {name} size={size} fill={fill} cull={cull} {dtype}: {counts.tolist()} chords, max ink err {err:.3e} "
          f"(bound {ink_atol(size):.3e}), mean ink {got.mean().item():.4f}")
    assert err <= ink_atol(size)
    assert 0.0 < got.mean().item() < 1.0 and got.min().item() >= 0.0 and got.max().item() <= 1.0
    if name == "gap":
        assert int(counts[1]) == 0 and bool((got[1] == 0).all()), "the image without chords is not exactly zero"
        assert bool(got[0].any()) and bool(got[2].any())
    assert torch.equal(ops.rasterize(c, a, size=size, fill=fill, n=10, groups=G, cull=cull).cpu(), got)


def test_analytic_square_on_the_device(gpu_device):
    commands, args = square()
    inside, edge, outside = square_masks()
    img = render.rasterize(commands.to(DEV), args.to(DEV), size=64, fill=True)[0].cpu()
    err = (img[edge] - 0.5).abs().max().item()
    print(f"filled square: edge pixels off 0.5 by {err:.3e}")
    assert bool((img[inside] == 1.0).all()) and bool((img[outside] == 0.0).all()) and err <= ink_atol(64)
    img = render.rasterize(commands.to(DEV), args.to(DEV), size=64, stroke_width=3.2)[0].cpu()
    err = (img[edge] - 0.9).abs().max().item()
    print(f"stroked square: line pixels off 0.9 by {err:.3e}")
    _, _, far = square_masks(lo=7, hi=25)
    assert err <= ink_atol(64) and bool((img[far] == 0).all()) and bool((img[9, 9:24] == 0).all())


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("size", [64, 100])
def test_culling_and_a_second_run_leave_every_bit_as_it_is(gpu_device, size, fill):
    for name, (commands, args, G) in _batches().items():
        c, a = _flat(commands, args, torch.float32)
        segs, counts = ops.raster_segments(c, a, n=10, groups=G, fill=fill)
        for width in (3.2, 0.0, 40.0):
            plain = ops.raster_sweep(segs, counts, size=size, stroke_width=width, fill=fill, cull=False)
            culled = ops.raster_sweep(segs, counts, size=size, stroke_width=width, fill=fill, cull=True)
            diff = (plain - culled).abs().max().item()
            print(f"{name} size={size} fill={fill} width={width}: max |cull=0 - cull=1| {diff:.3e}")
            assert torch.equal(plain.view(torch.int32), culled.view(torch.int32)), "culling changed the image"
            again = ops.raster_sweep(segs, counts, size=size, stroke_width=width, fill=fill, cull=False)
            assert torch.equal(plain.view(torch.int32), again.view(torch.int32)), "two runs differ in bits"
        segs2, counts2 = ops.raster_segments(c, a, n=10, groups=G, fill=fill)
        live = torch.arange(segs.shape[1], device=DEV).view(1, -1, 1) < counts.view(-1, 1, 1)
        assert torch.equal(counts, counts2) and torch.equal((segs.view(torch.int32) * live), (segs2.view(torch.int32) * live))


def test_rasterize_allocates_the_workspace_and_the_output_only(gpu_device):
    """16 icons of 8 x 32 tokens at 64 x 64: a [pixels, chords] matrix would be hundreds of MB, a copy of the inputs 393 KB"""
    commands, args = _random_sequences(16, 8, 32, seed=6)
    c, a = _flat(commands, args, torch.int64)
    for fill in (False, True):
        ops.rasterize(c, a, size=64, fill=fill, groups=8)                   # (code objects loaded)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = ops.rasterize(c, a, size=64, fill=fill, groups=8)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        budget = lib.load().dsvg_raster_workspace_bytes(16, 8, 32, 10, int(fill)) + out.numel() * 4
        print(f"rasterize fill={fill}: peak allocation grew by {grown} bytes, workspace + output {budget}")
        assert grown <= budget + (64 << 10) and bool(torch.isfinite(out).all())


# ---- reconstruction_images, interpolate ---------------------------------------------------------------------------------------
def _model(name):
    g, cfg, commands, args, _ = H.golden_setup(name)
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(H.weights_for(model, g["wseed"]))
    model.to(DEV)
    model.set_compute_dtype(torch.float32)
    return model, commands.to(DEV), args.to(DEV)


@pytest.mark.parametrize("name", ["hier_ordered_n5", "onestage50_n3"])
def test_reconstruction_images_and_interpolate(gpu_device, name):
    model, commands, args = _model(name)
    model.train()
    N = commands.shape[0]
    res = render.reconstruction_images(model, commands, args, size=32)
    assert model.training and res["decoded"].shape == (N, 32, 32) and res["target"].shape == (N, 32, 32)
    assert torch.equal(res["target"], render.rasterize(commands, args, size=32)) and bool(res["target"].any())
    model.eval()
    with torch.no_grad():
        cy, ay = model.greedy_sample(commands, args, commands, args, concat_groups=False, temperature=0.0)
        z = model(commands, args, None, None, encode_mode=True)                  # seq-first (1, 1, N, dim_z)
    assert torch.equal(res["decoded"], render.rasterize(cy, ay, size=32))
    # interpolate between latents that decode to something: with these seeded weights the encoded targets of the two-stage
    # golden decode to empty icons, and images without ink would make the equalities below hold for any rasteriser
    model.train()
    M = 16
    z1 = 3 * torch.randn(1, 1, M, z.shape[-1], generator=torch.Generator().manual_seed(1)).to(DEV)
    z2 = 3 * torch.randn(1, 1, M, z.shape[-1], generator=torch.Generator().manual_seed(4)).to(DEV)
    out = render.interpolate(model, z1, z2, steps=3, size=32)
    assert model.training and out["frames"].shape == (M, 3, 32, 32)
    assert torch.equal(out["frames"], render.rasterize(out["commands"].flatten(0, 1), out["args"].flatten(0, 1),
                                                       size=32).view(M, 3, 32, 32))
    model.eval()
    with torch.no_grad():
        c1, a1 = model.greedy_sample(None, None, None, None, z=z1.permute(2, 1, 0, 3), concat_groups=False, temperature=0.0)
    first = render.rasterize(c1, a1, size=32)
    inked = [int((out["frames"][:, k].flatten(1).amax(1) > 0).sum()) for k in range(3)]
    print(f"{name}: ink of the decoded icons {res['decoded'].mean().item():.4f}, of the targets {res['target'].mean().item():.4f}, "
          f"of frame 0 {first.mean().item():.4f}; icons with ink per frame {inked} of {M}")
    assert inked[0] > 0 and inked[2] > 0, "the latents decode to empty icons: the equalities would hold vacuously"
    assert torch.equal(out["commands"][:, 0], c1) and torch.equal(out["args"][:, 0], a1)
    assert torch.equal(out["frames"][:, 0].view(torch.int32), first.view(torch.int32))
    batch_first = render.interpolate(model, z1.permute(2, 1, 0, 3), z2.permute(2, 1, 0, 3), steps=3, size=32, fill=True)
    assert torch.equal(batch_first["commands"], out["commands"]) and batch_first["frames"].shape == (M, 3, 32, 32)
    assert bool(batch_first["frames"].any())
    # and between the encoded targets, seq-first as encode_mode hands them out
    enc = render.interpolate(model, z, z.flip(2), steps=3, size=32)
    with torch.no_grad():
        c1, a1 = model.greedy_sample(None, None, None, None, z=z.permute(2, 1, 0, 3), concat_groups=False, temperature=0.0)
    assert enc["frames"].shape == (N, 3, 32, 32) and torch.equal(enc["commands"][:, 0], c1) and torch.equal(enc["args"][:, 0], a1)
    assert torch.equal(enc["frames"][:, 0].view(torch.int32), render.rasterize(c1, a1, size=32).view(torch.int32))
