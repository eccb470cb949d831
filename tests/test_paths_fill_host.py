"""deepsvg_amd.paths.overlap / compute_filling without a GPU: the argument checks, the float64 restatement
(tests/paths_fill_ref.py) against the reference's own walk (tests/golden/paths/filling.npz, written by
tests/golden/make_golden_filling.py) and on hand cases whose answer is known, and the share of borderline samples on the
icons tests/test_paths_fill_gpu.py compares the device with.

Chord records come from tests/raster_layers_ref.raster_segments_layers here (the float64 chord list rounded to float32), on
the device from the segment kernel itself; the restatement takes either."""
import os
import re

import numpy as np
import pytest
import torch

from deepsvg_amd import lib, paths
from tests import paths_fill_ref as FR
from tests import raster_layers_ref as LR
from tests.test_draw_host import icon, ring
from tests.test_render_host import square

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTLINE, FILL, ERASE = FR.OUTLINE, FR.FILL, FR.ERASE

# (B, G, L, seed) of the curve icons, and the sample counts, of the device comparison
CURVE_SHAPES = [(3, 8, 12, 11), (2, 3, 66, 12), (1, 8, 256, 13)]
CURVE_SAMPLES = [8, 33, 64, 128]


def curve_icons(B, G, L, seed, dtype):
    """icons in the style of tests/test_metrics_gpu.py::_random_sequences (all seven commands, `l` and `c` half of the time,
    arguments from -1..255 in EVERY slot), with an empty group in the middle of every icon, at the end of the first and at the
    start of the last; float32: the same icons with a uniform fraction added to every argument"""
    gen = torch.Generator().manual_seed(seed)
    pool = torch.tensor([0, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6])
    commands = pool[torch.randint(0, len(pool), (B, G, L), generator=gen)]
    commands[:, G // 2] = 4
    commands[0, G - 1] = 4
    commands[B - 1, 0] = 4
    args = torch.randint(-1, 256, (B, G, L, 11), generator=gen)
    if dtype == torch.int64:
        return commands.long(), args.long()
    frac = torch.rand(args.shape, generator=torch.Generator().manual_seed(seed + 1000))
    return commands.float(), args.float() + frac


def records(commands, args, n=10):
    """commands [N, G, S], args [N, G, S, 11] -> (segs, seg_counts, layer_first) with every group's mode FILL, on the host"""
    N, G, S = commands.shape
    modes = torch.ones(N, G, dtype=torch.int32)
    return LR.raster_segments_layers(commands.reshape(N * G, S), args.reshape(N * G, S, 11), modes, n=n, groups=G)


def restated(commands, args, n=2, **kw):
    segs, seg_counts, layer_first = records(commands, args, n)
    return FR.compute_filling(segs.numpy(), seg_counts.numpy(), layer_first.numpy(), commands.numpy(), args.numpy(), **kw)


# ---- argument checks ---------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    commands, args = ring()
    ok = dict(samples=64)
    for fn in (paths.overlap, paths.compute_filling):
        for bad in (dict(samples=7), dict(samples=1025), dict(samples=64.0), dict(samples=True), dict(n=1), dict(n=65)):
            with pytest.raises(ValueError):
                fn(commands, args, **{**ok, **bad})
        with pytest.raises(ValueError, match="32"):
            fn(torch.zeros(1, 33, 4), torch.zeros(1, 33, 4, 11), **ok)
        with pytest.raises(ValueError, match="2048"):
            fn(torch.zeros(1, 32, 65), torch.zeros(1, 32, 65, 11), **ok)
        with pytest.raises(ValueError):
            fn(commands, args[:, :1], **ok)
        with pytest.raises(ValueError):
            fn(commands[0, 0], args[0, 0], **ok)
    for bad in (dict(rule="nonzero"), dict(rule=None), dict(threshold=0.0), dict(threshold=1.01), dict(threshold=-0.5),
                dict(threshold=float("nan")), dict(threshold="0.9"), dict(closed=torch.ones(1, 3, dtype=torch.bool)),
                dict(closed=torch.ones(2, dtype=torch.bool)), dict(closed=torch.ones(1, 2)), dict(closed=[[True, True]])):
        with pytest.raises(ValueError):
            paths.compute_filling(commands, args, **{**ok, **bad})


# ---- the reference's own walk ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "paths", "filling.npz"))
    adj = (g["adj"][:, :, None] >> np.arange(8, dtype=np.uint8)[None, None, :]) & 1          # adj[n, j, i]: an edge j -> i
    return {"adj": adj, "clockwise": g["clockwise"], "family": g["family"], "order_free": g["order_free"],
            "filling": g["filling"]}


def test_golden_file_holds_what_it_should(gold):
    free, fam = gold["order_free"], gold["family"]
    share = free[fam == 1].mean()
    print(f"order-free: {int(free.sum())} of {len(free)} cases; share of the random family {share:.4f}")
    assert bool(free[fam == 0].all()) and share >= 0.95
    assert (fam == 0).sum() >= 100 and (fam == 1).sum() >= 100
    assert (gold["filling"] == ERASE).any() and (gold["filling"] == OUTLINE).any()
    assert not bool(np.diagonal(gold["adj"], axis1=1, axis2=2).any())


def test_restatement_equals_the_reference_on_every_order_free_case(gold):
    worst = 0
    for k in np.nonzero(gold["order_free"])[0]:
        area, inter = FR.counts_from_adjacency(gold["adj"][k])
        got = FR.filling_from_counts(area, inter, gold["clockwise"][k], [True] * 8, 0.9, "orientation")
        worst = max(worst, int((np.array(got["filling"]) != gold["filling"][k]).sum()))
    print(f"groups whose filling differs from the reference's, worst case: {worst}")
    assert worst == 0


def test_order_free_is_what_the_file_says(gold):
    for k in range(0, len(gold["order_free"]), 7):
        area, inter = FR.counts_from_adjacency(gold["adj"][k])
        up, down = (FR.filling_from_counts(area, inter, gold["clockwise"][k], [True] * 8, 0.9, "orientation", order=o)
                    for o in ("ascending", "descending"))
        assert (up == down) == bool(gold["order_free"][k]), k


# ---- hand cases ---------------------------------------------------------------------------------------------------------
def test_ring():
    commands, args = ring()
    r = restated(commands, args, rule="evenodd")
    print("ring: area", r["area"].tolist(), "inter", r["inter"].tolist())
    assert r["area"].tolist() == [[1024, 256]] and r["inter"].tolist() == [[[1024, 256], [256, 256]]]
    assert r["clockwise"].tolist() == [[1, 1]]
    assert r["filling"].tolist() == [[FILL, ERASE]] and r["depth"].tolist() == [[0, 1]] and r["parent"].tolist() == [[-1, 0]]
    assert restated(commands, args, rule="orientation")["filling"].tolist() == [[FILL, FILL]]
    commands, args = icon(square(34, 98), square(50, 82, reverse=True))
    r = restated(commands, args, rule="orientation")
    assert r["clockwise"].tolist() == [[1, 0]] and r["filling"].tolist() == [[FILL, ERASE]]


def test_three_nested_squares():
    commands, args = icon(square(20, 120), square(40, 100), square(60, 80))
    for rule in ("evenodd", "orientation"):
        r = restated(commands, args, rule=rule)
        assert r["depth"].tolist() == [[0, 1, 2]] and r["parent"].tolist() == [[-1, 0, 1]]
    assert restated(commands, args, rule="evenodd")["filling"].tolist() == [[FILL, ERASE, FILL]]
    assert restated(commands, args, rule="orientation")["filling"].tolist() == [[FILL, FILL, FILL]]      # d = 1, 2, 3


def test_disjoint_identical_and_open_squares():
    r = restated(*icon(square(20, 60), square(100, 140)))
    assert r["filling"].tolist() == [[FILL, FILL]] and r["depth"].tolist() == [[0, 0]] and r["parent"].tolist() == [[-1, -1]]
    r = restated(*icon(square(34, 98), square(34, 98)))
    assert r["filling"].tolist() == [[OUTLINE, OUTLINE]] and r["depth"].tolist() == [[-1, -1]], "mutual cover: never reached"
    commands, args = ring()
    r = restated(commands, args, closed=np.array([[False, True]]))
    assert r["filling"].tolist() == [[OUTLINE, FILL]] and r["parent"].tolist() == [[-1, -1]]
    assert r["paint_order"].tolist() == [[1, 0]], "outlines are painted last"
    # a group without chords does not participate either
    empty = (torch.full((1, 8), 4.0), torch.full((1, 8, 11), -1.0))
    r = restated(*icon(square(34, 98), empty, square(50, 82)))
    assert r["filling"].tolist() == [[FILL, OUTLINE, ERASE]] and r["paint_order"].tolist() == [[0, 2, 1]]


def test_swapped_ring_is_painted_outer_first():
    commands, args = ring()
    r = restated(commands.flip(1), args.flip(1))
    assert r["filling"].tolist() == [[ERASE, FILL]] and r["depth"].tolist() == [[1, 0]] and r["parent"].tolist() == [[1, -1]]
    assert r["paint_order"].tolist() == [[1, 0]]


def test_clockwise_is_step_5_of_canonicalize():
    (c, a), (cr, ar) = square(), square(reverse=True)
    assert FR.is_clockwise(c[0], a[0]) and not FR.is_clockwise(cr[0], ar[0])
    one = torch.full((4,), 4.0)
    one[1] = 1.0
    arg = torch.full((4, 11), -1.0)
    arg[0, 9:], arg[1, 9:] = torch.tensor([5.0, 9.0]), torch.tensor([5.0, 9.0])
    assert FR.is_clockwise(one, arg)                      # one command, start == end
    arg[1, 9:] = torch.tensor([5.0, 8.0])
    assert not FR.is_clockwise(one, arg)
    assert FR.is_clockwise(torch.full((4,), 4.0), arg)    # no command at all: the empty sum is >= 0


# ---- borderline samples on the icons of the device comparison ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("shape", CURVE_SHAPES)
def test_borderline_samples_are_rare_on_the_curve_icons(shape, dtype):
    B, G, L, seed = shape
    commands, args = curve_icons(B, G, L, seed, dtype)
    segs, seg_counts, layer_first = records(commands, args, n=10)
    for samples in CURVE_SAMPLES:
        area, _, border = FR.overlap_counts(segs.numpy(), seg_counts.numpy(), layer_first.numpy(), samples)
        per_icon = np.diagonal(border, axis1=1, axis2=2).sum(1)              # >= the samples borderline for any group
        print(f"{shape} {dtype} samples={samples}: borderline per icon {per_icon.tolist()} of {samples * samples}; "
              f"inside some group: {area.sum(1).tolist()}")
        assert (per_icon <= 0.01 * samples * samples).all()
        assert (area.sum(1) > 0).all()


# ---- surface --------------------------------------------------------------------------------------------------------------
def test_package_and_binding_declare_the_ops():
    assert "overlap" in paths.__all__ and "compute_filling" in paths.__all__
    hdr = open(os.path.join(ROOT, "include", "dsvg.h")).read()
    assert lib.ABI_VERSION == int(re.search(r"#define DSVG_ABI_VERSION (\d+)", hdr).group(1))
    assert len(lib.SIGNATURES["dsvg_overlap_counts"][1]) == 11 and len(lib.SIGNATURES["dsvg_filling_from_counts"][1]) == 17
    assert lib.SIGNATURES["dsvg_filling_from_counts"][1][9] is lib.C.c_double
    assert (lib.DSVG_FILLING_EVENODD, lib.DSVG_FILLING_ORIENTATION) == (0, 1)
    for name, value in (("DSVG_FILLING_EVENODD", 0), ("DSVG_FILLING_ORIENTATION", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr)
    L = lib.load()
    assert L.dsvg_overlap_counts(None, None, None, 1, 1, 1, 64, 0, None, None, None) != 0
    assert b"overlap_counts: null pointer" in L.dsvg_last_error()
    # the limits are refused by the library too, before anything is launched (the pointers are never followed)
    p = 64
    for G, samples, word in ((33, 64, b"G = 33"), (8, 7, b"samples = 7"), (8, 1025, b"samples = 1025")):
        assert L.dsvg_overlap_counts(p, p, p, 1, 100, G, samples, 0, p, p, None) != 0
        assert b"overlap_counts" in L.dsvg_last_error() and word in L.dsvg_last_error()
    for G, thr, rule, word in ((33, 0.9, 0, b"G = 33"), (8, 0.0, 0, b"threshold"), (8, 1.5, 0, b"threshold"), (8, 0.9, 2, b"rule")):
        assert L.dsvg_filling_from_counts(0, p, p, p, p, p, 1, G, 4, thr, rule, p, p, p, p, p, None) != 0
        assert b"filling_from_counts" in L.dsvg_last_error() and word in L.dsvg_last_error()
