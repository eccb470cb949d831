"""deepsvg_amd.paths.split / arcs_to_beziers on the host: the float64 restatement (tests/paths_expand_ref.py) against what the
reference's own SVGPath.split and SVGPath.simplify_arcs returned (tests/golden/paths/expand.npz, written by
tests/golden/make_golden_paths_expand.py), the documented deviations on hand-made arcs, and the argument checks of both
functions with ops replaced.  No GPU: the kernel is compared with the restatement in tests/test_paths_expand_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from deepsvg_amd import lib, paths
from tests import paths_expand_ref as ER

M, L, C, A, EOS, SOS, Z = range(7)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths", "expand.npz")
SPLIT_VARIANTS = [("n1", dict(n=1)), ("n2", dict(n=2)), ("n5", dict(n=5)),
                  ("d2_lines", dict(max_dist=2 * 256 / 24, include_lines=True)),
                  ("d2_nolines", dict(max_dist=2 * 256 / 24, include_lines=False)),
                  ("d7_lines", dict(max_dist=7.5 * 256 / 24, include_lines=True)),
                  ("d7_nolines", dict(max_dist=7.5 * 256 / 24, include_lines=False))]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def against_reference(got, oc, oa, ln, bound, tags):
    """commands, counts and len_groups by equality, the enabled coordinates within `bound`, everything else framing"""
    assert got["valid"].all()
    assert np.array_equal(got["len_groups"], ln)
    worst = 0.0
    for b in range(len(ln)):
        for g in range(ln.shape[1]):
            n = ln[b, g]
            assert np.array_equal(got["commands"][b, g, 1:1 + n], oc[b, g, :n].astype(np.float32)), (tags[b], g)
            assert got["commands"][b, g, 0] == SOS and (got["commands"][b, g, 1 + n:] == EOS).all()
            assert (got["args"][b, g, 0] == -1).all() and (got["args"][b, g, 1 + n:] == -1).all()
            live = ER.enabled(got["commands"][b, g, 1:1 + n])
            assert (got["args"][b, g, 1:1 + n][~live] == -1).all()
            d = np.abs(got["args"][b, g, 1:1 + n].astype(np.float64) - oa[b, g, :n].astype(np.float64))[live]
            worst = max(worst, float(d.max(initial=0.0)))
    print(f"largest coordinate difference to the reference {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("name,kw", SPLIT_VARIANTS, ids=[v[0] for v in SPLIT_VARIANTS])
def test_split_restatement_equals_the_reference(gold, name, kw):
    oc, oa, ln = gold[f"split_{name}_commands"], gold[f"split_{name}_args"], gold[f"split_{name}_len"]
    got = ER.split(gold["split_commands"].astype(np.float32), gold["split_args"], max_seq_len=oc.shape[2], **kw)
    against_reference(got, oc, oa, ln, 2 * float(gold["split_max_abs_diff"]), gold["split_tags"])
    if name == "n1":                     # the identity
        assert np.array_equal(got["commands"], gold["split_commands"].astype(np.float32)[:, :, :oc.shape[2] + 2])


def test_split_lengths_are_the_references(gold):
    got = ER.split(gold["split_commands"].astype(np.float32), gold["split_args"], n=1)["lengths"].astype(np.float64)
    want = gold["split_lengths"]
    assert np.array_equal(got > 0, want > 0)
    # float32 out: 2^-24 relative, on top of what the generator measured between the float64 lengths
    is_c = gold["split_commands"] == C
    rel = np.abs(got - want) / np.maximum(want, 1.0)
    assert rel[is_c].max() <= 2.0 ** -24 + 2 * float(gold["length_max_rel_diff"])
    assert rel[~is_c].max() <= 2.0 ** -24 + 2 * float(gold["line_length_max_rel_diff"])


def test_arcs_restatement_equals_the_reference(gold):
    oc, oa, ln = gold["arcs_out_commands"], gold["arcs_out_args"], gold["arcs_out_len"]
    got = ER.arcs_to_beziers(gold["arcs_commands"].astype(np.float32), gold["arcs_args"], max_seq_len=oc.shape[2])
    against_reference(got, oc, oa, ln, 2 * float(gold["arcs_max_abs_diff"]), gold["arcs_tags"])
    assert not (got["commands"] == A).any()


def pieces_of(gold, tag):
    b = gold["arcs_tags"].tolist().index(tag)
    got = ER.arcs_to_beziers(gold["arcs_commands"][b:b + 1].astype(np.float32), gold["arcs_args"][b:b + 1], max_seq_len=30)
    return got, b


def test_golden_file_holds_the_cases_the_issue_names(gold):
    tags = gold["arcs_tags"].tolist()
    for tag in ["circle_two_semicircles", "quarter_arc", "three_quarter_arc", "rotated_ellipse", "both_radii_zero_dropped",
                "start_equals_end_dropped", "random"]:
        assert tag in tags, tag
    for tag, rows in [("circle_two_semicircles", [1] * 4 + [2] * 4), ("quarter_arc", [1, 1]), ("three_quarter_arc", [1] * 6)]:
        got, b = pieces_of(gold, tag)
        k = len(rows)                                                       # the pieces, behind the m (the circle: and a z)
        assert got["source_row"][0, 0, 2:2 + k].tolist() == [r + 1 for r in rows], tag
        assert (got["commands"][0, 0, :2 + k] == C).sum() == k == (gold["arcs_out_commands"][b, 0] == C).sum()
        assert got["commands"][0, 0, 2 + k] in (Z, EOS)
    for tag, n_arcs in [("both_radii_zero_dropped", 2), ("start_equals_end_dropped", 2)]:
        got, b = pieces_of(gold, tag)
        src = gold["arcs_commands"][b, 0]
        kept = [r for r in range(1, 16) if src[r] not in (EOS, A)]
        assert (src == A).sum() == n_arcs and got["source_row"][0, 0, 1:1 + len(kept)].tolist() == kept
    assert len(gold["split_tags"]) >= 30 and len(tags) >= 30 and (gold["arcs_commands"] == A).sum() >= 100
    for name, _ in SPLIT_VARIANTS:
        assert gold[f"split_{name}_len"].sum() > 300
    assert gold["split_commands"].shape[1:] == gold["arcs_commands"].shape[1:] == (4, 16)


# ---- the two deviations: against the geometry, not the reference -------------------------------------------------------
def one_arc(start, values, S=16):
    cmd = np.full((1, 1, S), EOS, np.float32)
    arg = np.full((1, 1, S, 11), -1.0, np.float32)
    cmd[0, 0, :3] = [SOS, M, A]
    arg[0, 0, 1, 9:11] = start
    arg[0, 0, 2, 0:5] = values[:5]
    arg[0, 0, 2, 9:11] = values[5:]
    return cmd, arg


@pytest.mark.parametrize("values", [[10, 10, 0, 0, 1, 100, 40], [5, 20, 30, 1, 0, 120, 200], [30, 8, -75, 1, 1, 20, 150],
                                    [-12, 3, 200, 0, 0, 200, 60]])
def test_radii_too_small_for_the_chord_are_scaled_up(values):
    start = (40.0, 50.0)
    cmd, arg = one_arc(start, values)
    par = ER.arc_parameters(*start, *[float(v) for v in values])
    assert par["lam"] > 1.0
    s = math.sqrt(par["lam"])
    assert par["rx"] == s * abs(values[0]) and par["ry"] == s * abs(values[1])
    # the chord is a diameter: the centre is its midpoint and the sweep half a turn, in the direction fS asks for
    assert abs(par["cx"] - 0.5 * (start[0] + values[5])) < 1e-12 and abs(par["cy"] - 0.5 * (start[1] + values[6])) < 1e-12
    assert par["dth"] == (180.0 if values[4] else -180.0) and par["k"] == 4
    # every piece lies on the scaled ellipse: its start, its end, and (a cubic approximates) its middle within 1e-3 of 1
    on = lambda x, y: ellipse_value(par, x, y)
    k = par["k"]
    pts = [start] + [tuple(ER.arc_piece(par, i)[4:6]) for i in range(k)]
    t1 = par["th1"] * ER.D2R
    p_first = (par["cx"] + par["cphi"] * par["rx"] * math.cos(t1) - par["sphi"] * par["ry"] * math.sin(t1),
               par["cy"] + par["sphi"] * par["rx"] * math.cos(t1) + par["cphi"] * par["ry"] * math.sin(t1))
    assert max(abs(p_first[0] - start[0]), abs(p_first[1] - start[1])) < 1e-9          # the first piece starts at the start
    assert max(abs(pts[-1][0] - values[5]), abs(pts[-1][1] - values[6])) < 1e-9        # the last ends at the end
    for x, y in pts:
        assert abs(on(x, y) - 1.0) < 1e-9
    for i in range(k):
        q = ER.arc_piece(par, i)
        mid = [ER.eval_cubic(pts[i][d], q[d], q[2 + d], q[4 + d], 0.5) for d in (0, 1)]
        assert abs(on(*mid) - 1.0) < 1e-3
    # and through the op: the written end is the input's end bit for bit
    got = ER.arcs_to_beziers(cmd, arg)
    assert got["valid"].all() and got["len_groups"][0, 0] == 1 + k and (got["commands"][0, 0, 2:2 + k] == C).all()
    assert np.array_equal(got["args"][0, 0, 1 + k, 9:11], arg[0, 0, 2, 9:11])


def ellipse_value(par, x, y):
    """((x, y) - centre) rotated back by phi, over the radii, squared and summed: 1 on the ellipse"""
    ux, uy = x - par["cx"], y - par["cy"]
    xr, yr = par["cphi"] * ux + par["sphi"] * uy, par["cphi"] * uy - par["sphi"] * ux
    return (xr / par["rx"]) ** 2 + (yr / par["ry"]) ** 2


@pytest.mark.parametrize("values", [[0, 30, 0, 0, 1, 100, 40], [25, 0, 45, 1, 0, 7, 9], [-0.0, 3, 10, 1, 1, 200, 60]])
def test_exactly_one_zero_radius_gives_a_line(values):
    cmd, arg = one_arc((40.0, 50.0), values)
    assert ER.arc_parameters(40.0, 50.0, *[float(v) for v in values]) == ER.LINE
    got = ER.arcs_to_beziers(cmd, arg)
    assert got["valid"].all() and got["len_groups"][0, 0] == 2
    assert got["commands"][0, 0, :4].tolist() == [SOS, M, L, EOS] and got["source_row"][0, 0, :4].tolist() == [-1, 1, 2, -1]
    assert np.array_equal(got["args"][0, 0, 2], np.array([-1] * 9 + values[5:], np.float32))


def test_restatement_rules_around_the_geometry():
    cmd, arg = ER.random_icons(6, 3, 12, seed=5)
    ident = ER.split(cmd, arg, n=1)
    assert ident["valid"].all() and np.array_equal(ident["commands"], cmd)
    assert np.array_equal(ident["args"], np.where(ER.enabled(cmd), arg, np.float32(-1)))
    far = ER.split(cmd, arg, max_dist=1e6)
    assert all(np.array_equal(far[k], ident[k]) for k in ident)
    # a group filled to exactly S_out - 2 rows is valid, one more row is not - for that icon alone
    n_rows = (cmd[:, :, 1:] != EOS).sum(-1)
    longest = int(n_rows.max())
    fit = ER.split(cmd, arg, n=1, max_seq_len=longest)
    assert fit["valid"].all() and fit["len_groups"].max() == longest
    tight = ER.split(cmd, arg, n=1, max_seq_len=longest - 1)
    assert np.array_equal(tight["valid"], n_rows.max(1) <= longest - 1) and not tight["valid"].all() and tight["valid"].any()
    bad = ~tight["valid"]
    assert (tight["len_groups"][bad] == 0).all() and (tight["source_row"][bad] == -1).all()
    assert (tight["commands"][bad][:, :, 0] == SOS).all() and (tight["commands"][bad][:, :, 1:] == EOS).all()
    # an arc under split, a NaN on a live row: that icon alone; garbage behind the first EOS: nothing
    c2, a2 = cmd.copy(), arg.copy()
    b, g = np.argwhere(n_rows >= 2)[0]
    c2[b, g, 2] = A
    res = ER.split(c2, a2, n=2, max_seq_len=40)
    assert not res["valid"][b] and res["valid"].sum() == len(cmd) - 1
    c3, a3 = cmd.copy(), arg.copy()
    a3[cmd == EOS] = np.nan
    a3[:, :, -1][cmd[:, :, -1] == EOS] = 3e38
    res3, base = ER.split(c3, a3, n=2, max_seq_len=40), ER.split(cmd, arg, n=2, max_seq_len=40)
    assert all(np.array_equal(res3[k], base[k]) for k in base)


# ---- the public functions: argument checks before the device is touched --------------------------------------------
class _FakeOps:
    def __init__(self):
        self.calls = []

    def paths_expand(self, commands, args, s_out, **mode):
        self.calls.append((commands, args, s_out, mode))
        N, G, S = commands.shape
        res = {"commands": torch.zeros(N, G, s_out), "args": torch.zeros(N, G, s_out, 11),
               "len_groups": torch.zeros(N, G, dtype=torch.int32), "source_row": torch.zeros(N, G, s_out, dtype=torch.int32),
               "valid": torch.ones(N, dtype=torch.bool)}
        if not mode.get("arcs"):
            res["lengths"] = torch.zeros(N, G, S)
        return res


@pytest.fixture
def fake_ops(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(paths.ops, "paths_expand", fake.paths_expand, raising=True)
    return fake


def test_split_checks_its_arguments(fake_ops):
    c3, a3 = torch.zeros(2, 8, 32), torch.zeros(2, 8, 32, 11)
    for kw in [dict(), dict(n=2, max_dist=3.0), dict(n=0), dict(n=-1), dict(n=2.0), dict(n=True), dict(max_dist=0.0),
               dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")), dict(max_dist="7")]:
        with pytest.raises(ValueError, match="split"):
            paths.split(c3, a3, **kw)
    for bad in [(c3, a3[:, :, :31]), (c3, a3[..., :10]), (c3[0, 0], a3[0, 0]), (c3[None], a3[None]), (c3, a3[:1]),
                (c3[:0], a3[:0])]:
        with pytest.raises(ValueError, match="split"):
            paths.split(*bad, n=2)
        with pytest.raises(ValueError, match="arcs_to_beziers"):
            paths.arcs_to_beziers(*bad)
    with pytest.raises(ValueError, match="2048"):
        paths.split(torch.zeros(1, 8, 257), torch.zeros(1, 8, 257, 11), n=2)
    with pytest.raises(ValueError, match="2048"):
        paths.split(c3, a3, n=2, max_seq_len=255)                          # 8 x 257 rows out
    with pytest.raises(ValueError, match="2048"):
        paths.arcs_to_beziers(c3, a3, max_seq_len=255)
    with pytest.raises(ValueError, match="max_seq_len"):
        paths.arcs_to_beziers(c3, a3, max_seq_len=-1)
    assert not fake_ops.calls                                              # none of them reached the device


def test_shapes_dtypes_and_defaults(fake_ops):
    c3, a3 = torch.zeros(2, 8, 32), torch.zeros(2, 8, 32, 11, requires_grad=True)
    res = paths.split(c3, a3, n=3)
    c, a, s_out, mode = fake_ops.calls.pop()
    assert s_out == 32 and mode == dict(n=3, max_dist=0.0, include_lines=True) and not a.requires_grad
    assert sorted(res) == ["args", "commands", "len_groups", "lengths", "source_row", "valid"]
    paths.split(c3, a3, max_dist=7.5, include_lines=False, max_seq_len=100)
    assert fake_ops.calls.pop()[2:] == (102, dict(n=0, max_dist=7.5, include_lines=False))
    res = paths.arcs_to_beziers(c3.long()[:, 0], a3.detach().long()[:, 0], max_seq_len=60)     # (N, S), int64 as greedy_sample
    c, a, s_out, mode = fake_ops.calls.pop()
    assert c.shape == (2, 1, 32) and a.shape == (2, 1, 32, 11) and c.dtype == a.dtype == torch.float32 and c.is_contiguous()
    assert s_out == 62 and mode == dict(arcs=True) and "lengths" not in res
    assert res["commands"].shape == (2, 62) and res["args"].shape == (2, 62, 11) and res["len_groups"].shape == (2,)
    assert res["source_row"].shape == (2, 62) and res["valid"].shape == (2,)


def test_package_and_binding_declare_the_op():
    assert {"split", "arcs_to_beziers"} <= set(paths.__all__)
    assert len(lib.SIGNATURES["dsvg_paths_expand"][1]) == 17 and (lib.DSVG_EXPAND_SPLIT, lib.DSVG_EXPAND_ARCS) == (0, 1)
