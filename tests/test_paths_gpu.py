"""deepsvg_amd.paths.canonicalize on the device (csrc/paths.hip) against the float64 restatement (tests/paths_ref.py) and the
reference's own results (tests/golden/paths/canonicalize.npz): equality on all seven outputs - every output value is a copy of
an input value, only the decisions are computed.  The restatement is compared with the reference in tests/test_paths_host.py."""
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import metrics, paths
from deepsvg_amd.synthetic import make_batch, make_batch_onestage
from tests import metrics_ref as MR
from tests import paths_ref as PR

pytestmark = pytest.mark.gpu

KEYS = ("commands", "args", "n_groups", "len_groups", "source_group", "reversed", "valid")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths", "canonicalize.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def check(dev, cmd, arg, only=None, **kw):
    """kernel == restatement on all seven outputs (icons `only`, a bool mask, where given) -> the kernel's dict"""
    cmd_t = cmd if torch.is_tensor(cmd) else torch.from_numpy(cmd)
    arg_t = arg if torch.is_tensor(arg) else torch.from_numpy(arg)
    got = paths.canonicalize(cmd_t.to(dev), arg_t.to(dev), **kw)
    want = PR.canonicalize(cmd_t.cpu().numpy(), arg_t.cpu().numpy(), **kw)
    assert tuple(got) == KEYS
    for key in KEYS:
        g, w = got[key].cpu(), torch.from_numpy(want[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
        if only is not None:
            g, w = g[only], w[only]
        if not torch.equal(g, w):
            bad = [b for b in range(g.shape[0]) if not torch.equal(g[b], w[b])]
            raise AssertionError(f"{key}: {len(bad)} of {g.shape[0]} icons differ from the restatement, first {bad[:8]}")
    return got


@pytest.mark.parametrize("num", [None, 256])
@pytest.mark.parametrize("layout", ["grouped", "concat"])
@pytest.mark.parametrize("dtype", ["float32", "int64"])
def test_golden_icons(gpu_device, gold, dtype, layout, num):
    sel = np.ones(len(gold["tags"]), bool)
    if dtype == "int64":                        # the icons with float coordinates have no int64 form
        sel = np.array([not str(t).startswith("float") for t in gold["tags"]])
    dt = np.dtype(dtype)
    g_out, max_len, want = PR.golden_expected(gold, layout, rounded=num is not None, dtype=dt)
    got = check(gpu_device, gold["commands"][sel].astype(dt), gold["args"][sel].astype(dt), max_num_groups=g_out,
                max_seq_len=max_len, layout=layout, numericalize=num)
    assert bool(got["valid"].all())
    for key, exp in want.items():               # and the reference itself
        assert torch.equal(got[key].cpu(), torch.from_numpy(exp[sel])), key


def test_golden_icons_at_tight_limits(gpu_device, gold):
    """max_num_groups and max_seq_len below what some icons need: the valid / overflow rules on the device"""
    cmd, arg = gold["commands"].astype(np.float32), gold["args"]
    for kw in ({"max_num_groups": 3, "max_seq_len": 5}, {"max_num_groups": 2, "max_seq_len": 9, "layout": "concat"},
               {"max_num_groups": 1, "max_seq_len": 0}):
        got = check(gpu_device, cmd, arg, **kw)
        share = float(got["valid"].float().mean())
        assert 0.02 < share < 0.98, share           # both outcomes occur


@pytest.mark.parametrize("layout", ["grouped", "concat"])
def test_limits_exactly_reached_and_exceeded_by_one(gpu_device, layout):
    from tests.test_paths_host import M, SQUARE, icon
    cmd, arg = icon([SQUARE + [(M, [50, 60])] + SQUARE[1:]])        # two sub-paths of 4 rows in one input group
    fit = 4 if layout == "grouped" else 8
    got = check(gpu_device, cmd, arg, max_num_groups=2, max_seq_len=fit, layout=layout)
    assert got["valid"].tolist() == [True] and got["len_groups"].tolist() == [[4, 4]]
    for kw in ({"max_num_groups": 1, "max_seq_len": fit}, {"max_num_groups": 2, "max_seq_len": fit - 1}):
        got = check(gpu_device, cmd, arg, layout=layout, **kw)
        assert got["valid"].tolist() == [False] and got["n_groups"].tolist() == [0] and bool((got["args"] == -1).all())


def test_an_arc_before_the_first_eos_makes_the_icon_invalid(gpu_device):
    from tests.test_paths_host import A, EOS, SQUARE, icon
    cmd, arg = icon([SQUARE + [(A, [])], SQUARE])
    cmd, arg = np.concatenate([cmd, cmd, cmd]), np.concatenate([arg, arg, arg])
    cmd[1, 0, 5], cmd[1, 1, 6] = EOS, A                               # icon 1: the arc behind its group's first EOS
    cmd[2, 0, 5], cmd[2, 0, 0] = EOS, A                               # icon 2: an arc in place of the SOS
    got = check(gpu_device, cmd, arg)
    assert got["valid"].tolist() == [False, True, False] and got["n_groups"].tolist() == [0, 2, 0]


def test_already_canonical_icon_comes_back_unchanged(gpu_device, gold):
    b = gold["tags"].tolist().index("already_canonical")
    cmd = torch.from_numpy(gold["commands"][b:b + 1].astype(np.float32)).to(gpu_device)
    arg = torch.from_numpy(gold["args"][b:b + 1]).to(gpu_device)
    got = paths.canonicalize(cmd, arg)
    assert torch.equal(got["commands"], cmd) and torch.equal(got["args"], arg) and not bool(got["reversed"].any())
    got = paths.canonicalize(cmd.long(), arg.long(), numericalize=256)
    assert torch.equal(got["commands"], cmd.long()) and torch.equal(got["args"], arg.long())


def test_two_stage_batch(gpu_device):
    cmd, arg = make_batch(37, G=8, S=30, seed=4)
    got = check(gpu_device, cmd, arg)
    assert bool(got["valid"].all()) and int(got["n_groups"].max()) == 8 and bool(got["reversed"].any())
    check(gpu_device, cmd, arg, layout="concat", max_seq_len=240, numericalize=256)
    check(gpu_device, cmd, arg, layout="concat")                    # 30 rows in all: most icons do not fit
    check(gpu_device, cmd.long(), arg.long(), max_num_groups=6, max_seq_len=25)


def test_one_stage_batch_of_256_rows(gpu_device):
    """254 commands + SOS + EOS: four waves of rows, sub-paths that straddle the 64-row boundaries"""
    cmd, arg = make_batch_onestage(19, total_len=254, seed=2)
    assert cmd.shape == (19, 1, 256)
    got = check(gpu_device, cmd[:, 0], arg[:, 0], max_num_groups=8, max_seq_len=254, layout="concat")
    assert bool(got["valid"].any()) and got["commands"].shape == (19, 256)
    m_rows = (cmd[:, 0] == 0).nonzero()[:, 1]
    assert any(int(r) % 64 > 40 for r in m_rows)                    # a sub-path that starts late in a wave and crosses into the next
    check(gpu_device, cmd, arg, max_num_groups=8, max_seq_len=254)
    check(gpu_device, cmd[:, 0].long(), arg[:, 0].long(), max_num_groups=5, max_seq_len=100, numericalize=256)


def test_icons_of_2048_rows(gpu_device):
    cmd, arg = make_batch(3, G=8, S=254, seed=6, min_groups=8)
    assert cmd.shape == (3, 8, 256)
    got = check(gpu_device, cmd, arg)
    assert bool(got["valid"].all()) and int(got["len_groups"].max()) > 200
    # z and m rows sprinkled in: hundreds of sub-paths per icon
    g = torch.Generator().manual_seed(1)
    r = torch.rand(cmd.shape, generator=g)
    body = cmd < 3
    cmd2 = torch.where(body & (r < 0.15), torch.zeros_like(cmd), torch.where(body & (r > 0.93), torch.full_like(cmd, 6.0), cmd))
    arg2 = torch.where((cmd2 == 0).unsqueeze(-1) & (torch.arange(11) < 9), torch.full_like(arg, -1.0), arg)
    arg2 = torch.where((cmd2 == 6).unsqueeze(-1), torch.full_like(arg, -1.0), arg2)
    got = check(gpu_device, cmd2, arg2, max_num_groups=1024, max_seq_len=40)
    assert int(got["n_groups"].max()) > 100
    got = check(gpu_device, cmd2, arg2, max_num_groups=1024, max_seq_len=2046, layout="concat")
    assert bool(got["valid"].all())
    with pytest.raises(ValueError):
        paths.canonicalize(torch.zeros(1, 8, 257, device=gpu_device), torch.zeros(1, 8, 257, 11, device=gpu_device))


def test_a_single_icon(gpu_device):
    cmd, arg = make_batch(1, G=8, S=30, seed=9)
    check(gpu_device, cmd, arg)
    check(gpu_device, cmd[:, :1, :3], arg[:, :1, :3])               # SOS, m, l (or c) and nothing else


def test_random_float_icons_where_rounding_cannot_decide(gpu_device):
    """float32 coordinates uniform in [0, 256): compared where every closeness test is outside [0.5, 2] x its threshold and
    every determinant sum is at least 1e-4 of its terms' magnitudes; at most 5 % of the batch may fall outside (asserted on
    the same generator in tests/test_paths_host.py, where only the restatement runs)"""
    cmd, arg = PR.random_float_icons(200, seed=3)
    only = PR.decisive(cmd, arg)
    assert 1.0 - only.mean() <= 0.05
    check(gpu_device, cmd, arg, only=torch.from_numpy(only), max_num_groups=16)
    check(gpu_device, cmd, arg, only=torch.from_numpy(only), max_num_groups=16, max_seq_len=60, layout="concat",
          numericalize=256)


def test_two_calls_give_identical_bits(gpu_device):
    cmd, arg = make_batch(64, G=8, S=30, seed=12, device=gpu_device)
    a, b = paths.canonicalize(cmd, arg), paths.canonicalize(cmd, arg)
    for key in KEYS:
        x, y = a[key], b[key]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_capture_and_replay(gpu_device):
    cmd, arg = make_batch(16, G=8, S=30, seed=13, device=gpu_device)
    cmd_b, arg_b = make_batch(16, G=8, S=30, seed=14, device=gpu_device)
    want_a, want_b = paths.canonicalize(cmd, arg, numericalize=256), paths.canonicalize(cmd_b, arg_b, numericalize=256)
    sc, sa = cmd.clone(), arg.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        paths.canonicalize(sc, sa, numericalize=256)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = paths.canonicalize(sc, sa, numericalize=256)
    for want, (c, a) in ((want_a, (cmd, arg)), (want_b, (cmd_b, arg_b)), (want_a, (cmd, arg))):
        sc.copy_(c)
        sa.copy_(a)
        graph.replay()
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(out[key], want[key]), key


@pytest.fixture(scope="module")
def geometry(gpu_device):
    """-> measure(n): over the icons of make_batch(37, 8, 30) where nothing is dropped and no closed sub-path has a gap (all
    37; 95 of their 175 sub-paths come back reversed), the Chamfer distance between the clouds of n points per command of
    the input and of its canonical form: by the device (metrics.sample_points, metrics.chamfer) and by their float64
    restatement (tests/metrics_ref.py).  Canonicalised once, measured once per n."""
    cmd, arg = make_batch(37, G=8, S=30, seed=4)
    facts = PR.icon_facts(cmd.numpy(), arg.numpy())
    keep = torch.tensor([clean and not arc for clean, arc in facts])
    assert int(keep.sum()) >= 30
    got = paths.canonicalize(cmd.to(gpu_device), arg.to(gpu_device))
    assert bool(got["valid"].all()) and int(got["reversed"].sum()) >= 20
    oc, oa = got["commands"].cpu(), got["args"].cpu()
    assert bool((oc == 2).any(-1)[got["reversed"].cpu()].any())                 # reversed sub-paths with `c` commands
    done = {}

    def measure(n):
        if n not in done:
            dev = metrics.chamfer(*metrics.sample_points(cmd.to(gpu_device), arg.to(gpu_device), n=n),
                                  *metrics.sample_points(got["commands"], got["args"], n=n)).cpu()
            ref = MR.chamfer(*MR.sample_points(cmd.reshape(-1, 32), arg.reshape(-1, 32, 11), n=n, groups=8),
                             *MR.sample_points(oc.reshape(-1, 32), oa.reshape(-1, 32, 11), n=n, groups=8), as_double=True)
            print(f"n = {n}: chamfer(input, output): device max {float(dev[keep].max()):.3e} mean "
                  f"{float(dev[keep].mean()):.3e}; float64 restatement max {float(ref[keep].max()):.3e} mean "
                  f"{float(ref[keep].mean()):.3e}; {int(got['reversed'].sum())} of {int(got['n_groups'].sum())} sub-paths reversed")
            done[n] = (dev[keep].double(), ref[keep])
        return done[n]
    return measure


@pytest.mark.parametrize("n", [5, 9])
def test_geometry_is_preserved(geometry, n):
    """Where nothing is dropped and no closed sub-path has a gap the output draws the input's curves: the Chamfer distance
    between the point clouds of input and output is at most 4 x what the float64 restatement of sample_points
    (tests/metrics_ref.py) gives for the same pair.

    What the restatement gives is exactly 0, at every n: it evaluates in float64 and rounds its points to float32, and from
    either end of a command it lands on the same float32.  So the bound is 0, and the number of points per command, which
    the check leaves open, is chosen where the device's fp32 sampler can be held to it: at n = 5 and n = 9 the parameters
    z = k / (n - 1) are multiples of 1/4 and 1/8, and with integer arguments below 256 every step of the sampler is exact
    (`l`: fma(z, p3 - p0, p0), a multiple of 1/8 below 256; `c`: the power basis has integer coefficients below 4096, the
    three Horner steps give multiples of 1/8, 1/64, 1/512 below 4096: 21 bits of the 24).  Exact points do not depend on
    the end a command is evaluated from, so input and output give the same point set and the distance is exactly 0 - unless
    a row was copied wrongly: z = 1/4 and 1/8 tell a reversed `c` whose control points were not swapped from one whose were
    (z = 1/2 alone would not).  Measured on an MI355X, n = 5 and n = 9: device max 0.0, restatement max 0.0.  At the
    default n = 10, where z is rounded, the device gives max 1.085e-05, mean 5.553e-06 (a third of an ulp at 256) against
    the same 0: test_geometry_is_preserved_to_fp32_rounding bounds that by the number format."""
    dev, ref = geometry(n)
    assert bool((dev <= 4 * ref).all()), (float(dev.max()), float(ref.max()))


def test_geometry_is_preserved_to_fp32_rounding(geometry):
    """The same distance at the default n = 10, where z = k / 9 is rounded, against a bound from the number format.  A cloud
    point is a Horner evaluation in fp32 of the power basis with |c_i| <= 3 * 4 * 255 = 3060 < 4096: three fused multiply-adds,
    each rounding a value below 4096 * 3 (ulp 9.8e-4 at most, half of it per rounding, damped by z <= 1 on the way out): below
    3 * 4.9e-4 = 1.5e-3 per coordinate.  Input and output evaluate the same exact point, so corresponding points are within
    2 * sqrt(2) * 1.5e-3 = 4.2e-3 of each other, and the two directed means of the Chamfer distance sum to at most 8.4e-3.  A
    reversal that kept the control points in place, or a wrong start point, moves points by whole units.  (Measured: max
    1.1e-5, mean 5.6e-6.)"""
    dev, _ = geometry(10)
    assert bool((dev <= 8.4e-3).all()), float(dev.max())
