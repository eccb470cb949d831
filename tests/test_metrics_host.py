"""deepsvg_amd.metrics on CPU: the plain-torch restatements of the two ops (tests/metrics_ref.py) against the reference's
golden (tests/golden/metrics/metrics_points.npz, make_golden_metrics.py), and the host logic of sample_points / chamfer /
reconstruction_error with the ops replaced by restatements.

Tolerances: a coefficient sum of the cubic reaches 8 * 255 ~ 2048, where half an fp32 ulp is 1.2e-4; the reference's fp32
result carries four such terms: 5e-4 on points.  A distance of at most 362 from exact fp32 differences carries a few ulps:
1e-4 on the Chamfer distance (the golden's is float64)."""
import math
import os

import numpy as np
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import metrics
from tests import helpers as H
from tests import metrics_ref as MR

GOLDEN = os.path.join(H.GOLDEN_DIR, "metrics", "metrics_points.npz")
POINT_ATOL, CHAMFER_ATOL = 5e-4, 1e-4


@pytest.fixture
def metric_ops(emulated_ops):
    saved = MR.install()
    yield
    MR.restore(saved)


def golden():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    return g, torch.from_numpy(g["commands"]), torch.from_numpy(g["args"])


def check_points_against_golden(g, n, points, counts):
    """-> max abs error; counts exact, points to POINT_ATOL up to counts[i]"""
    off, want = g[f"off_n{n}"], torch.from_numpy(g[f"pts_n{n}"])
    assert counts.tolist() == np.diff(off).tolist()
    worst = 0.0
    for i in range(len(off) - 1):
        err = (points[i, :counts[i]].double() - want[off[i]:off[i + 1]].double()).abs().max().item()
        worst = max(worst, err)
    assert worst <= POINT_ATOL, f"n={n}: points off by {worst:.3e}"
    return worst


@pytest.mark.parametrize("n", [2, 7, 10])
def test_restated_sample_points_match_the_reference(n):
    g, commands, args = golden()
    points, counts = MR.sample_points(commands, args, n=n)
    assert points.shape == (commands.shape[0], commands.shape[1] * (n - 1) + 1, 2) and counts.dtype == torch.int32
    check_points_against_golden(g, n, points, counts)
    # int64 inputs, as greedy_sample returns them
    p2, c2 = MR.sample_points(commands.long(), args.long(), n=n)
    assert torch.equal(p2, points) and torch.equal(c2, counts)


def test_restated_chamfer_matches_the_reference():
    g, commands, args = golden()
    points, counts = MR.sample_points(commands, args, n=10)
    i, j = torch.from_numpy(g["pairs"]).long().unbind(1)
    got = MR.chamfer(points[i], counts[i], points[j], counts[j], as_double=True)
    err = (got - torch.from_numpy(g["chamfer"])).abs().max().item()
    assert err <= CHAMFER_ATOL, err
    assert torch.equal(MR.chamfer(points, counts, points, counts), torch.zeros(len(counts)))


def test_cloud_of_an_icon_is_the_concatenation_of_its_groups(metric_ops):
    g, commands, args = golden()
    N, G, S = 3, 4, commands.shape[1]
    commands, args = commands.clone(), args.clone()
    commands[5] = 4.0                                   # an empty group in the middle of icon 1 ...
    args[5] = -1.0
    commands[11] = 4.0                                  # ... and one at the end of icon 2
    args[11] = -1.0
    for n in (2, 10):
        rows_p, rows_c = metrics.sample_points(commands, args, n=n)
        assert rows_c[5] == 0 and rows_c[11] == 0
        icon_p, icon_c = metrics.sample_points(commands.view(N, G, S), args.view(N, G, S, 11), n=n)
        assert icon_p.shape == (N, G * (S * (n - 1) + 1), 2)
        assert icon_c.tolist() == rows_c.view(N, G).sum(1).tolist()
        for i in range(N):
            want = torch.cat([rows_p[i * G + k, :rows_c[i * G + k]] for k in range(G)])
            assert torch.equal(icon_p[i, :icon_c[i]], want)


def test_empty_clouds_give_count_zero_and_nan(metric_ops):
    commands = torch.tensor([[5, 0, 6, 4, 4], [4, 4, 4, 4, 4], [5, 0, 1, 4, 4]], dtype=torch.float32)   # no l / c in rows 0, 1
    args = torch.randint(0, 256, (3, 5, 11), generator=torch.Generator().manual_seed(0)).float()
    p, c = metrics.sample_points(commands, args, n=10)
    assert c.tolist() == [0, 0, 10]
    full_p, full_c = p[2:3].expand(3, -1, -1).contiguous(), c[2:3].expand(3).contiguous()
    for got in (metrics.chamfer(p, c, full_p, full_c), metrics.chamfer(full_p, full_c, p, c)):
        assert torch.isnan(got[:2]).all() and got[2] == 0
    assert torch.isnan(metrics.chamfer(p, c, p, c)[:2]).all()


def test_sample_points_refuses_other_layouts(metric_ops):
    with pytest.raises(ValueError):
        metrics.sample_points(torch.zeros(4), torch.zeros(4, 11))
    with pytest.raises(ValueError):
        metrics.sample_points(torch.zeros(2, 4), torch.zeros(2, 5, 11))


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("name", ["hier_ordered_n5", "onestage50_n3"])
def test_reconstruction_error_host_logic(name, training, metric_ops):
    """(with these seeded weights the two-stage model decodes no drawing command: its icons are all invalid; the one-stage
    fixture gives finite errors)"""
    g, cfg, commands, args, _ = H.golden_setup(name)
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(H.weights_for(model, g["wseed"]))
    model.train(training)
    decoded = {}
    greedy = model.greedy_sample

    def spy(*a, **k):
        decoded["kw"] = k
        decoded["out"] = greedy(*a, **k)
        return decoded["out"]
    model.greedy_sample = spy
    res = metrics.reconstruction_error(model, commands, args)
    assert model.training == training
    assert decoded["kw"] == dict(label=None, concat_groups=False, temperature=0.0)
    cy, ay = decoded["out"]
    N = commands.shape[0]
    assert cy.shape[0] == N and cy.dtype == torch.int64 and ay.dtype == torch.int64
    # re == the restatement applied to that call's own decoded tensors and to the targets as passed
    px, nx = MR.sample_points(cy.reshape(-1, cy.shape[-1]), ay.reshape(-1, *ay.shape[-2:]), 10, groups=cy.shape[1])
    py, ny = MR.sample_points(commands.reshape(-1, commands.shape[-1]), args.reshape(-1, *args.shape[-2:]), 10,
                              groups=commands.shape[1])
    want = MR.chamfer(px, nx, py, ny)
    assert res["re"].shape == (N,) and res["re"].dtype == torch.float32
    valid = (nx > 0) & (ny > 0)
    assert res["valid"].dtype == torch.bool and torch.equal(res["valid"], valid) and bool(ny.gt(0).all())
    assert torch.equal(torch.isnan(res["re"]), ~valid)
    assert torch.equal(res["re"][valid], want[valid]) and bool(valid.any()) == (name == "onestage50_n3")
    assert res["mean"].dim() == 0
    if bool(valid.any()):
        assert math.isclose(res["mean"].item(), res["re"][valid].double().mean().item(), rel_tol=1e-6)
        assert bool((res["re"][valid] >= 0).all())
    else:
        assert math.isnan(res["mean"].item())


def test_reconstruction_error_of_the_targets_is_zero(metric_ops):
    g, cfg, commands, args, _ = H.golden_setup("hier_ordered_n5")
    model = deepsvg_amd.SVGTransformer(cfg)
    model.greedy_sample = lambda *a, **k: (commands.long(), args.long())
    res = metrics.reconstruction_error(model, commands, args, n=7)
    assert bool(res["valid"].all()) and torch.equal(res["re"], torch.zeros(commands.shape[0])) and res["mean"].item() == 0
