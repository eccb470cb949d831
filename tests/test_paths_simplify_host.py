"""deepsvg_amd.paths.simplify / simplify_heuristic on the host: the float64 restatement (tests/paths_simplify_ref.py) against what
the reference's own SVGPath.simplify and SVGPath.simplify_heuristic returned (tests/golden/paths/simplify.npz, written by
tests/golden/make_golden_paths_simplify.py), what the definition promises of a result, the invalid cases, and the argument
checks of both functions with ops replaced.  No GPU: the kernel is compared with the restatement in
tests/test_paths_simplify_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import lib, paths
from tests import paths_simplify_ref as SR

M, L, C, A, EOS, SOS, Z = range(7)
UNIT = 256 / 24
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths", "simplify.npz")
VARIANTS = [("fit", dict(tolerance=0.1, epsilon=0.2, angle_threshold=150.0)), ("default", {}), ("smooth", dict(force_smooth=True))]
CRAFTED = ["one_line", "polyline", "one_long_cubic", "c_l_c_sharp_corners", "closed_with_z", "smooth_s_curve", "empty_group"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def padded_input(gold, name):
    """the int8 rows of the file, padded with -2, as the (N, G, S) layout: SOS, rows, EOS"""
    oc, oa, ln = gold[f"{name}_commands"], gold[f"{name}_args"], gold[f"{name}_len"]
    n, g, lo = oc.shape
    cmd = np.full((n, g, lo + 2), EOS, np.float32)
    arg = np.full((n, g, lo + 2, 11), -1.0, np.float32)
    cmd[:, :, 0] = SOS
    live = np.arange(lo)[None, None] < ln[..., None]
    cmd[:, :, 1:1 + lo][live] = oc[live]
    arg[:, :, 1:1 + lo][live] = oa[live]
    return cmd, arg


def against_reference(got, oc, oa, ln, bound):
    """commands and len_groups by equality, the enabled coordinates within `bound` reference units"""
    assert got["valid"].all()
    assert np.array_equal(got["len_groups"], ln)
    worst = 0.0
    for b in range(len(ln)):
        for g in range(ln.shape[1]):
            n = ln[b, g]
            assert np.array_equal(got["commands"][b, g, 1:1 + n], oc[b, g, :n].astype(np.float32)), (b, g)
            assert got["commands"][b, g, 0] == SOS and (got["commands"][b, g, 1 + n:] == EOS).all()
            live = SR.enabled(got["commands"][b, g, 1:1 + n])
            assert (got["args"][b, g, 1:1 + n][~live] == -1).all() and (got["args"][b, g, 1 + n:] == -1).all()
            d = np.abs(got["args"][b, g, 1:1 + n].astype(np.float64) - oa[b, g, :n].astype(np.float64))[live] / UNIT
            worst = max(worst, float(d.max(initial=0.0)))
    print(f"largest coordinate difference to the reference {worst:.3e} reference units, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_simplify_restatement_equals_the_reference(gold, name, kw):
    cmd, arg = padded_input(gold, "pre")
    oc, oa, ln = gold[f"{name}_commands"], gold[f"{name}_args"], gold[f"{name}_len"]
    got = SR.simplify(cmd, arg, max_seq_len=oc.shape[2], **kw)
    against_reference(got, oc, oa, ln, 2 * float(gold["simplify_max_abs_diff"]))


def test_simplify_heuristic_restatement_equals_the_reference(gold):
    oc, oa, ln = gold["heuristic_commands"], gold["heuristic_args"], gold["heuristic_len"]
    got = SR.simplify_heuristic(gold["commands"].astype(np.float32), gold["args"], max_seq_len=oc.shape[2])
    against_reference(got, oc, oa, ln, 2 * float(gold["simplify_max_abs_diff"]))


def test_golden_file_holds_the_named_cases(gold):
    tags = set(gold["tags"].ravel())
    assert set(CRAFTED) <= tags
    assert gold["commands"].shape[1:] == (4, 48) and gold["commands"].shape[0] >= 40
    assert (gold["rejected_share"] <= 0.5).all() and 0 < float(gold["simplify_max_abs_diff"]) < 1e-2
    s = np.argwhere(gold["tags"] == "smooth_s_curve")[0]
    assert gold["pre_len"][s[0], s[1]] > 64                           # more than 64 points after the split
    families = set(gold["family"].ravel())
    assert {"crafted", "short", "long"} <= families
    assert os.path.getsize(GOLD) < 256 * 1024


@pytest.fixture(scope="module")
def batch():
    cmd, arg = SR.random_batch(3, 4, 80, seed=1)
    return cmd, arg, SR.simplify(cmd, arg, 0.1, 0.2, 150.0)


def test_properties_of_the_restatements_result(batch):
    cmd, arg, out = batch
    assert out["valid"].all()
    n_c, n_l = SR.check_properties(cmd, arg, out, 0.1, 0.2)
    assert n_c >= 10 and n_l >= 1                                     # the batch holds both kinds
    out = SR.simplify(cmd, arg, force_smooth=True)
    assert SR.check_properties(cmd, arg, out, 0.1, 0.1)[0] >= 10


def test_a_group_can_grow_and_empty_gaps_are_zero_length_lines():
    cmd, arg = SR.pack([[SR.GROWS, SR.CORNER]], 2, 12)
    out = SR.simplify(cmd, arg, 0.1, 0.2, 150.0)
    assert out["valid"][0] and list(out["len_groups"][0]) == [8, 8]
    assert list(out["commands"][0, 0, 1:9]) == [M, L, C, L, C, L, C, L]
    assert list(out["source_row"][0, 0, 1:9]) == [1, 1, 2, 2, 3, 3, 4, 4]
    assert list(out["commands"][0, 1, 1:9]) == [M, L, C, L, C, L, C, L]
    assert list(out["source_row"][0, 1, 1:9]) == [1, 1, 2, 3, 4, 4, 5, 5]
    SR.check_properties(cmd, arg, out, 0.1, 0.2)


def invalid_batch():
    """icon 0 and 4 are fine; 1: two coincident consecutive points in a fitted run; 2: a live `a`; 3: a NaN"""
    good = SR.pieces([20, 30, 200, 40, 30, 180, 220, 200], 6)
    twice = [good[0], (C, good[1][1][:4] + good[0][1])] + good[1:]    # a `c` that ends where it starts: no direction at the run's start
    arc = good[:3] + [(A, [20.0, 20.0, 0.0, 0.0, 1.0, 90.0, 90.0])]
    nan = good[:2] + [(C, [float("nan")] + good[2][1][1:])] + good[3:]
    return SR.pack([[good], [twice], [arc], [nan], [good]], 1, 12)


def test_invalid_cases_make_that_icon_alone_invalid():
    cmd, arg = invalid_batch()
    out = SR.simplify(cmd, arg, 0.1, 0.2, 150.0)
    assert list(out["valid"]) == [True, False, False, False, True]
    for b in (1, 2, 3):
        assert out["len_groups"][b].sum() == 0 and (out["commands"][b, :, 1:] == EOS).all() and (out["args"][b] == -1).all()
        assert (out["source_row"][b] == -1).all()
    assert np.array_equal(out["args"][0], out["args"][4]) and out["len_groups"][0, 0] > 0


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"ops.{name} reached: the argument checks come before the device")


def test_argument_checks(monkeypatch):
    monkeypatch.setattr(paths, "ops", _NoDevice())
    cmd, arg = torch.zeros(2, 4, 16), torch.zeros(2, 4, 16, 11)
    for kw in (dict(tolerance=0.0), dict(tolerance=math.nan), dict(tolerance=math.inf), dict(epsilon=-1.0), dict(epsilon=math.nan),
               dict(angle_threshold=-1.0), dict(angle_threshold=180.5), dict(angle_threshold=math.nan), dict(unit=0.0),
               dict(unit=math.inf), dict(max_seq_len=-1), dict(max_seq_len=2048 // 4 - 1)):
        with pytest.raises(ValueError, match="^simplify: "):
            paths.simplify(cmd, arg, **kw)
    with pytest.raises(ValueError, match="^simplify: "):
        paths.simplify(cmd, arg[..., :10])
    with pytest.raises(ValueError, match="^simplify: "):
        paths.simplify(torch.zeros(1, 2, 1025), torch.zeros(1, 2, 1025, 11))
    for kw in (dict(unit=0.0), dict(unit=math.nan), dict(max_seq_len=-1), dict(max_seq_len=511), dict(work_seq_len=511),
               dict(work_seq_len=1.5)):
        with pytest.raises(ValueError, match="^simplify_heuristic: "):
            paths.simplify_heuristic(cmd, arg, **kw)
    with pytest.raises(ValueError, match="^simplify_heuristic: "):
        paths.simplify_heuristic(cmd, arg[..., :10])
    with pytest.raises(ValueError, match="^simplify_heuristic: "):
        paths.simplify_heuristic(torch.zeros(4), torch.zeros(4, 11))


def test_the_op_is_declared():
    assert "simplify" in paths.__all__ and "simplify_heuristic" in paths.__all__
    res, argtypes = lib.SIGNATURES["dsvg_paths_simplify"]
    assert len(argtypes) == 19 and "dsvg_paths_simplify_workspace_bytes" in lib.SIGNATURES
    assert lib.ABI_VERSION == 19
    assert "stays on the host" not in paths.__doc__ and "simplify_heuristic" in paths.__doc__
