"""deepsvg_amd.paths.split / arcs_to_beziers on the device (csrc/paths_expand.hip) against the float64 restatement
(tests/paths_expand_ref.py).  split: equality on every output, "lengths" included - its arithmetic is float64 with no library
function but the square root.  arcs_to_beziers: commands, counts and source rows by equality, coordinates within one float32
ulp (two correct float64 evaluations with different sin / cos / tan / acos can round to neighbouring float32 values and no
further).  The restatement is compared with the reference in tests/test_paths_expand_host.py."""
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import paths
from tests import paths_expand_ref as ER

pytestmark = pytest.mark.gpu

M, L, C, A, EOS, SOS, Z = range(7)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths", "expand.npz")
SPLIT_KEYS = ("commands", "args", "len_groups", "source_row", "valid", "lengths")
ARC_KEYS = SPLIT_KEYS[:5]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def differing(g, w):
    return [b for b in range(g.shape[0]) if not np.array_equal(g[b], w[b])]


def check_split(dev, cmd, arg, **kw):
    """kernel == restatement on all six outputs -> (the kernel's dict as numpy, the restatement's)"""
    got = paths.split(torch.from_numpy(cmd).to(dev), torch.from_numpy(arg).to(dev), **kw)
    want = ER.split(cmd, arg, **kw)
    assert tuple(got) == SPLIT_KEYS
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for key in SPLIT_KEYS:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = differing(g, w)
            raise AssertionError(f"{key}: {len(bad)} of {len(g)} icons differ from the restatement, first {bad[:8]}; largest "
                                 f"difference {np.nanmax(np.abs(g.astype(np.float64) - w.astype(np.float64)))}")
    return got, want


def check_arcs(dev, cmd, arg, **kw):
    """kernel == restatement: args within one float32 ulp of the expected value, everything else equal"""
    got = paths.arcs_to_beziers(torch.from_numpy(cmd).to(dev), torch.from_numpy(arg).to(dev), **kw)
    want = ER.arcs_to_beziers(cmd, arg, **kw)
    assert tuple(got) == ARC_KEYS
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for key in ARC_KEYS:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
        if key == "args":
            ulps = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
            print(f"arcs: {int((g != w).sum())} of {g.size} values differ, by at most {ulps.max():.2f} ulp")
            assert np.isfinite(g).all() and ulps.max() <= 1.0
        else:
            assert np.array_equal(g, w), (key, differing(g, w)[:8])
    return got, want


# ---- the golden icons ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(n=1), dict(n=2), dict(n=5), dict(max_dist=2 * 256 / 24), dict(max_dist=7.5 * 256 / 24),
                                dict(max_dist=2 * 256 / 24, include_lines=False),
                                dict(max_dist=7.5 * 256 / 24, include_lines=False)],
                         ids=["n1", "n2", "n5", "d2_lines", "d7_lines", "d2_nolines", "d7_nolines"])
def test_split_golden_icons(gpu_device, gold, kw):
    got, _ = check_split(gpu_device, gold["split_commands"].astype(np.float32), gold["split_args"], max_seq_len=40, **kw)
    assert got["valid"].all()


def test_arcs_golden_icons(gpu_device, gold):
    got, _ = check_arcs(gpu_device, gold["arcs_commands"].astype(np.float32), gold["arcs_args"], max_seq_len=30)
    assert got["valid"].all() and not (got["commands"] == A).any()
    assert np.array_equal(got["len_groups"], gold["arcs_out_len"])                 # and the reference's own counts


# ---- seeded batches at the shapes where the scan can go wrong ----------------------------------------------------------
#         N, G, S, share of the rows in use at most, max_seq_len, max_dist
SHAPES = {"3x4x80": (3, 4, 80, 0.3, 200, 60.0),          # 320 rows: across a 256-thread chunk and wave boundaries
          "1x8x256": (1, 8, 256, 0.3, 254, 150.0),       # all 2,048 rows in, all 2,048 out
          "5x50": (5, 1, 50, 0.5, 400, 60.0)}            # the one-stage form (N, S)


def batch(shape, arcs):
    N, G, S, fill, max_seq_len, _ = SHAPES[shape]
    cmd, arg = ER.random_icons(N, G, S, seed=11 + len(shape) + arcs, arcs=arcs, fill=fill)
    if G == 1:
        cmd, arg = cmd[:, 0], arg[:, 0]
    return cmd, arg, max_seq_len


@pytest.fixture(scope="module")
def split_runs():
    return {}


@pytest.mark.parametrize("by", ["n", "max_dist"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_split_seeded_batches(gpu_device, split_runs, shape, by):
    cmd, arg, max_seq_len = batch(shape, arcs=False)
    kw = dict(n=3) if by == "n" else dict(max_dist=SHAPES[shape][5])
    got, _ = check_split(gpu_device, cmd, arg, max_seq_len=max_seq_len, **kw)
    assert got["valid"].all() and got["len_groups"].max() > (cmd != EOS).sum(-1).max()     # rows were added
    split_runs[shape, by] = (cmd, arg, got)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_arcs_seeded_batches(gpu_device, shape):
    cmd, arg, max_seq_len = batch(shape, arcs=True)
    got, _ = check_arcs(gpu_device, cmd, arg, max_seq_len=max_seq_len)
    assert got["valid"].any() and (cmd == A).sum() > 10 and not (got["commands"] == A).any()


def test_split_preserves_the_geometry(gpu_device, split_runs):
    """every piece, evaluated in float64 at z in {0, 1/2, 1}, is the source curve at (i + z) / k within 1e-4.  Derived: inside
    the 0..256 box a piece's control points are convex combinations of the source's, each rounded once to float32 (half an
    ulp of a value below 256: 1.6e-5), and evaluating a cubic is again a convex combination of its control points; the start
    of a piece is the rounded end of the piece before it"""
    key = ("3x4x80", "max_dist")
    if key not in split_runs:
        cmd, arg, max_seq_len = batch("3x4x80", arcs=False)
        got = {k: v.cpu().numpy() for k, v in paths.split(torch.from_numpy(cmd).to(gpu_device), torch.from_numpy(arg).to(
            gpu_device), max_dist=60.0, max_seq_len=max_seq_len).items()}
        split_runs[key] = (cmd, arg, got)
    cmd, arg, got = split_runs[key]
    worst, pieces = 0.0, 0
    for b, g in np.argwhere(got["len_groups"] > 0):
        oc, oa, src = got["commands"][b, g], got["args"][b, g].astype(np.float64), got["source_row"][b, g]
        r = 1
        while r <= got["len_groups"][b, g]:
            t = src[r]
            k = int((src == t).sum())
            if oc[r] in (L, C):
                ia = arg[b, g, t].astype(np.float64)
                p = [arg[b, g, t - 1, 9:11].astype(np.float64), ia[5:7], ia[7:9], ia[9:11]]
                if oc[r] == L:
                    p[1], p[2] = (2 * p[0] + p[3]) / 3, (p[0] + 2 * p[3]) / 3          # the line as a cubic
                for i in range(k):
                    row = oa[r + i]
                    q = [oa[r + i - 1, 9:11], row[5:7], row[7:9], row[9:11]]
                    if oc[r] == L:
                        q[1], q[2] = (2 * q[0] + q[3]) / 3, (q[0] + 2 * q[3]) / 3
                    for z in (0.0, 0.5, 1.0):
                        for d in (0, 1):
                            have = ER.eval_cubic(q[0][d], q[1][d], q[2][d], q[3][d], z)
                            want = ER.eval_cubic(p[0][d], p[1][d], p[2][d], p[3][d], (i + z) / k)
                            worst = max(worst, abs(have - want))
                    pieces += 1
            r += k
    print(f"{pieces} pieces, largest distance to the source curve {worst:.3e}")
    assert pieces > 300 and worst <= 1e-4


# ---- edges ----------------------------------------------------------------------------------------------------------
def test_edges(gpu_device):
    cmd, arg = ER.random_icons(6, 3, 12, seed=5)
    n_rows = (cmd[:, :, 1:] != EOS).sum(-1)
    cmd[1, 1, 1:], arg[1, 1, 1:] = EOS, -1                                   # a group of only SOS / EOS
    n_rows[1, 1] = 0
    ident, _ = check_split(gpu_device, cmd, arg, n=1)                      # n = 1 returns the input
    assert ident["valid"].all() and np.array_equal(ident["commands"], cmd)
    assert np.array_equal(ident["args"], np.where(ER.enabled(cmd), arg, np.float32(-1)))
    assert ident["len_groups"][1, 1] == 0 and np.array_equal(ident["len_groups"], n_rows)
    far, _ = check_split(gpu_device, cmd, arg, max_dist=1e6)                # max_dist above every length too
    assert all(np.array_equal(far[k], ident[k]) for k in SPLIT_KEYS)
    # a group filled to exactly S_out - 2 rows is valid; one more row makes that icon alone invalid
    longest = int(n_rows.max())
    fit, _ = check_split(gpu_device, cmd, arg, n=1, max_seq_len=longest)
    assert fit["valid"].all() and fit["len_groups"].max() == longest
    tight, _ = check_split(gpu_device, cmd, arg, n=1, max_seq_len=longest - 1)
    assert np.array_equal(tight["valid"], n_rows.max(1) <= longest - 1) and tight["valid"].any() and not tight["valid"].all()
    bad = ~tight["valid"]
    assert (tight["len_groups"][bad] == 0).all() and (tight["source_row"][bad] == -1).all()
    assert (tight["commands"][bad][:, :, 0] == SOS).all() and (tight["commands"][bad][:, :, 1:] == EOS).all()
    assert (tight["args"][bad] == -1).all()
    # the same through the counts: n = 2 doubles the l / c rows
    drawing = ((cmd == L) | (cmd == C)).sum(-1)
    twice, _ = check_split(gpu_device, cmd, arg, n=2, max_seq_len=int((n_rows + drawing).max()))
    assert twice["valid"].all() and np.array_equal(twice["len_groups"], n_rows + drawing)
    over, _ = check_split(gpu_device, cmd, arg, n=2, max_seq_len=int((n_rows + drawing).max()) - 1)
    assert np.array_equal(over["valid"], (n_rows + drawing).max(1) <= (n_rows + drawing).max() - 1) and over["valid"].any()
    # garbage behind the first EOS changes nothing
    base, _ = check_split(gpu_device, cmd, arg, n=3, max_seq_len=40)
    c2, a2 = cmd.copy(), arg.copy()
    first_eos = (cmd == EOS).argmax(-1)                                     # (every group has one)
    dead = np.arange(cmd.shape[2])[None, None] > first_eos[..., None]       # the rows behind it
    c2[dead] = np.tile(np.array([L, C, A, M, 77, np.nan, -3, 3e38], np.float32), dead.sum() // 8 + 1)[:dead.sum()]
    a2[dead] = np.nan
    a2[dead, 9] = 3e38
    a2[cmd == EOS] = np.where(dead[cmd == EOS][:, None], a2[cmd == EOS], np.float32(-np.inf))   # and on the first EOS row
    junk, _ = check_split(gpu_device, c2, a2, n=3, max_seq_len=40)
    assert dead.sum() > 50 and all(np.array_equal(junk[k], base[k]) for k in SPLIT_KEYS)
    junk, _ = check_arcs(gpu_device, c2, a2, max_seq_len=40)
    assert junk["valid"].all()
    # a NaN in a live row makes that icon alone invalid; so does a live `a` under split
    b, g = np.argwhere(((cmd[:, :, 2] == L) | (cmd[:, :, 2] == C)))[0]
    for col, val in [(9, np.nan), (10, np.inf), (9, -np.inf)]:
        a3 = arg.copy()
        a3[b, g, 2, col] = val
        res, _ = check_split(gpu_device, cmd, a3, n=2, max_seq_len=40)
        assert not res["valid"][b] and res["valid"].sum() == len(cmd) - 1
        res, _ = check_arcs(gpu_device, cmd, a3, max_seq_len=40)
        assert not res["valid"][b] and res["valid"].sum() == len(cmd) - 1
    c3, a3 = cmd.copy(), arg.copy()
    c3[b, g, 2], a3[b, g, 2, 0:5] = A, [30, 40, 10, 0, 1]
    res, _ = check_split(gpu_device, c3, a3, max_dist=50.0, max_seq_len=40)
    assert not res["valid"][b] and res["valid"].sum() == len(cmd) - 1
    res, _ = check_arcs(gpu_device, c3, a3, max_seq_len=40)
    assert res["valid"].all()
    # a cubic of length 0 gives one piece
    c4 = np.full((1, 1, 7), EOS, np.float32)
    a4 = np.full((1, 1, 7, 11), -1, np.float32)
    c4[0, 0, :4] = [SOS, M, C, L]
    a4[0, 0, 1, 9:11], a4[0, 0, 2, 5:11], a4[0, 0, 3, 9:11] = 7, 7, (7, 9.5)
    res, _ = check_split(gpu_device, c4, a4, max_dist=1.0)
    assert res["valid"].all() and res["commands"][0, 0].tolist() == [SOS, M, C, L, L, L, EOS]
    assert res["lengths"][0, 0, 3] == 2.5 and res["lengths"][0, 0, 2] < 1e-12
    assert res["source_row"][0, 0].tolist() == [-1, 1, 2, 3, 3, 3, -1]


def test_deviations_on_the_device(gpu_device):
    """radii too small for the chord, exactly one radius 0, negative radii, flags other than 0 / 1"""
    rows = [[10, 10, 0, 0, 1, 100, 40], [5, 20, 30, 1, 0, 120, 200], [30, 8, -75, 1, 1, 20, 150], [-12, 3, 200, 0, 0, 200, 60],
            [0, 30, 0, 0, 1, 100, 40], [25, 0, 45, 1, 0, 7, 9], [-60, -90, 15, 2, -1, 90, 120], [0, 0, 0, 0, 0, 9, 9]]
    cmd = np.full((len(rows), 1, 16), EOS, np.float32)
    arg = np.full((len(rows), 1, 16, 11), -1, np.float32)
    cmd[:, 0, :4] = [SOS, M, A, L]
    arg[:, 0, 1, 9:11], arg[:, 0, 3, 9:11] = (40, 50), (1, 2)
    arg[:, 0, 2, 0:5], arg[:, 0, 2, 9:11] = np.array(rows)[:, :5], np.array(rows)[:, 5:]
    got, _ = check_arcs(gpu_device, cmd, arg)
    assert got["valid"].all() and got["len_groups"][:, 0].tolist() == [6, 6, 6, 6, 3, 3, got["len_groups"][6, 0], 2]
    assert got["commands"][4, 0, :5].tolist() == [SOS, M, L, L, EOS]
    for b in range(7):                           # the last piece carries the end position bit for bit
        n = got["len_groups"][b, 0]
        assert np.array_equal(got["args"][b, 0, n - 1, 9:11], arg[b, 0, 2, 9:11])


# ---- composition and reproducibility ---------------------------------------------------------------------------------
def circle_batch(n, G, S, seed):
    """m, then lines and circular arcs (rx = ry: circles and rounded corners, what raw SVG is full of), some closed"""
    rng = np.random.default_rng(seed)
    cmd = np.full((n, G, S), EOS, np.float32)
    arg = np.full((n, G, S, 11), -1.0, np.float32)
    cmd[:, :, 0] = SOS
    for b in range(n):
        for g in range(G):
            rows = int(rng.integers(2, S - 2))
            at = rng.uniform(40, 216, 2)
            cmd[b, g, 1], arg[b, g, 1, 9:11] = M, at
            for r in range(2, 1 + rows):
                to = np.clip(at + rng.uniform(-90, 90, 2), 0, 255)
                if rng.random() < 0.5:
                    cmd[b, g, r] = L
                else:
                    cmd[b, g, r] = A
                    rad = 0.5 * np.hypot(*(to - at)) * rng.uniform(1.1, 2.0) + 1.0
                    arg[b, g, r, 0:5] = [rad, rad, 0, rng.integers(0, 2), rng.integers(0, 2)]
                arg[b, g, r, 9:11] = to
                at = arg[b, g, r, 9:11].astype(np.float64)
            if rng.random() < 0.5:
                cmd[b, g, 1 + rows] = Z
    return cmd, arg


def test_chain_back_into_the_model(gpu_device):
    cmd, arg = circle_batch(8, 2, 10, seed=3)
    dev = gpu_device
    c, a = torch.from_numpy(cmd).to(dev), torch.from_numpy(arg).to(dev)
    alone = paths.canonicalize(c, a, max_num_groups=4, max_seq_len=300, numericalize=256)
    assert ((cmd == A).any((1, 2)) == ~alone["valid"].cpu().numpy()).all() and not alone["valid"].any()
    no_arcs = paths.arcs_to_beziers(c, a, max_seq_len=70)
    assert bool(no_arcs["valid"].all()) and not bool((no_arcs["commands"] == A).any())
    short = paths.split(no_arcs["commands"], no_arcs["args"], max_dist=80.0, max_seq_len=300)
    assert bool(short["valid"].all())
    canon = paths.canonicalize(short["commands"], short["args"], max_num_groups=4, max_seq_len=300, numericalize=256)
    assert bool(canon["valid"].all()) and int(canon["n_groups"].min()) >= 1
    # no l / c of the split's result is longer than 80: its own lengths, taken again on the result
    again = paths.split(short["commands"], short["args"], n=1, max_seq_len=300)
    longest = float(again["lengths"].max())
    print(f"longest command after split(max_dist=80): {longest:.4f}; before: {float(short['lengths'].max()):.2f}")
    assert float(short["lengths"].max()) > 80.0 and longest <= 80.0
    assert torch.equal(again["commands"], short["commands"]) and torch.equal(again["args"], short["args"])


def test_two_calls_are_bit_identical(gpu_device):
    cmd, arg, max_seq_len = batch("3x4x80", arcs=True)
    c, a = torch.from_numpy(cmd).to(gpu_device), torch.from_numpy(arg).to(gpu_device)
    first, second = paths.arcs_to_beziers(c, a, max_seq_len=max_seq_len), paths.arcs_to_beziers(c, a, max_seq_len=max_seq_len)
    assert all(torch.equal(first[k].view(torch.int32) if first[k].dtype == torch.float32 else first[k],
                           second[k].view(torch.int32) if second[k].dtype == torch.float32 else second[k]) for k in first)
    s1 = paths.split(first["commands"], first["args"], max_dist=40.0, max_seq_len=max_seq_len)
    s2 = paths.split(first["commands"], first["args"], max_dist=40.0, max_seq_len=max_seq_len)
    assert all(torch.equal(s1[k].view(torch.int32) if s1[k].dtype == torch.float32 else s1[k],
                           s2[k].view(torch.int32) if s2[k].dtype == torch.float32 else s2[k]) for k in s1)
