"""deepsvg_amd.paths on the host: the float64 restatement (tests/paths_ref.py) against what the reference's own
SVG.canonicalize() returned (tests/golden/paths/canonicalize.npz, written by tests/golden/make_golden_paths.py), the rules
the restatement adds around it (valid / overflow, numericalize, source_group / reversed), and the argument checks of
paths.canonicalize with ops replaced.  No GPU: the kernel is compared with the restatement in tests/test_paths_gpu.py."""
import os

import numpy as np
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import lib, paths
from tests import paths_ref as PR

M, L, C, A, EOS, SOS, Z = range(7)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paths", "canonicalize.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def icon(groups, G=None, S=None, dtype=np.float32):
    """groups: lists of (command, values) -> commands [1, G, S], args [1, G, S, 11] with SOS / EOS framing"""
    G = G or max(len(groups), 1)
    S = S or max([len(g) for g in groups] + [1]) + 2
    cmd = np.full((1, G, S), EOS, dtype)
    arg = np.full((1, G, S, 11), -1, dtype)
    cmd[:, :, 0] = SOS
    for g, seq in enumerate(groups):
        for r, (c, v) in enumerate(seq, 1):
            cmd[0, g, r] = c
            if c in (M, L):
                arg[0, g, r, 9:11] = v
            elif c == C:
                arg[0, g, r, 5:11] = v
    return cmd, arg


@pytest.mark.parametrize("rounded", [False, True])
@pytest.mark.parametrize("layout", ["grouped", "concat"])
def test_restatement_equals_the_reference_on_every_golden_icon(gold, layout, rounded):
    g_out, max_len, want = PR.golden_expected(gold, layout, rounded)
    got = PR.canonicalize(gold["commands"].astype(np.float32), gold["args"], max_num_groups=g_out, max_seq_len=max_len,
                          layout=layout, numericalize=256 if rounded else None)
    assert got["valid"].all()
    for key, exp in want.items():
        bad = [str(gold["tags"][b]) for b in range(len(exp)) if not np.array_equal(got[key][b], exp[b])]
        assert not bad, f"{key}: {len(bad)} icons differ from the reference, first {bad[:5]}"
    assert got["commands"].dtype == got["args"].dtype == np.float32


def test_golden_file_holds_the_cases_the_kernel_can_get_wrong(gold):
    tags = set(gold["tags"].tolist())
    for tag in ["m_l_only", "empty_icon", "rows_before_m_and_after_z", "three_subpaths_in_a_group",
                "subpath_of_degenerate_commands_only", "degenerate_bezier_loop", "one_command_subpaths_both_orientations",
                "equal_start_keys_stable_order", "determinant_sum_zero", "reversed_start_breaks_sort_order",
                "closed_without_gap_rotated", "closed_with_gap_rotated", "c_commands_reversed", "float_coordinates",
                "already_canonical", "random"]:
        assert tag in tags, tag
    assert len(gold["norm_pairs"]) >= 4 and sum(t.startswith("norm32_") for t in tags) >= 4
    assert len(gold["tags"]) >= 200 and os.path.getsize(GOLD) < 256 * 1024
    # the fp32 norm decides those icons: a restatement with float64 norms gets at least four of them wrong
    _, _, want = PR.golden_expected(gold, "grouped")
    saved = PR._norm32
    PR._norm32 = lambda x, y: np.sqrt(np.float64(x) * x + np.float64(y) * y)
    try:
        sel = [b for b, t in enumerate(gold["tags"]) if str(t).startswith("norm32_")]
        got = PR.canonicalize(gold["commands"][sel].astype(np.float32), gold["args"][sel], max_num_groups=8, max_seq_len=14)
    finally:
        PR._norm32 = saved
    wrong = sum(not np.array_equal(got["args"][i], want["args"][b]) for i, b in enumerate(sel))
    assert wrong >= 4


def test_already_canonical_icon_comes_back_unchanged(gold):
    b = gold["tags"].tolist().index("already_canonical")
    cmd, arg = gold["commands"][b:b + 1].astype(np.float32), gold["args"][b:b + 1]
    got = PR.canonicalize(cmd, arg)
    assert np.array_equal(got["commands"], cmd) and np.array_equal(got["args"], arg)
    assert not got["reversed"].any() and got["source_group"][0].tolist() == [0, 1, 2, -1]


def test_int64_icons_give_the_same_rows(gold):
    sel = [b for b, t in enumerate(gold["tags"]) if not str(t).startswith("float")]
    cmd, arg = gold["commands"][sel], gold["args"][sel]
    f = PR.canonicalize(cmd.astype(np.float32), arg, max_num_groups=8, max_seq_len=14, layout="concat")
    i = PR.canonicalize(cmd.astype(np.int64), arg.astype(np.int64), max_num_groups=8, max_seq_len=14, layout="concat")
    assert i["commands"].dtype == i["args"].dtype == np.int64
    for key in f:
        assert np.array_equal(f[key], i[key]), key


SQUARE = [(M, [10, 10]), (L, [40, 10]), (L, [40, 40]), (L, [10, 40])]        # 4 rows, clockwise


@pytest.mark.parametrize("layout", ["grouped", "concat"])
def test_valid_at_the_limits_and_one_past_them(layout):
    # two sub-paths of 4 rows in ONE input group
    cmd, arg = icon([SQUARE + [(M, [50, 60])] + SQUARE[1:]])
    fit = 4 if layout == "grouped" else 8
    ok = PR.canonicalize(cmd, arg, max_num_groups=2, max_seq_len=fit, layout=layout)
    assert ok["valid"].tolist() == [True] and ok["n_groups"].tolist() == [2] and ok["len_groups"].tolist() == [[4, 4]]
    assert ok["commands"].shape[-1] == fit + 2 and ok["source_group"].tolist() == [[0, 0]]
    for kw in ({"max_num_groups": 1, "max_seq_len": fit}, {"max_num_groups": 2, "max_seq_len": fit - 1}):
        bad = PR.canonicalize(cmd, arg, layout=layout, **kw)
        assert bad["valid"].tolist() == [False] and bad["n_groups"].tolist() == [0]
        assert not bad["len_groups"].any() and (bad["source_group"] == -1).all() and not bad["reversed"].any()
        assert (bad["commands"][..., 0] == SOS).all() and (bad["commands"][..., 1:] == EOS).all() and (bad["args"] == -1).all()


def test_an_arc_before_the_first_eos_makes_the_icon_invalid_and_one_behind_it_does_not():
    cmd, arg = icon([SQUARE + [(A, [])], SQUARE])
    assert PR.canonicalize(cmd, arg)["valid"].tolist() == [False]
    cmd[0, 0, 5], cmd[0, 1, 5] = EOS, EOS
    cmd[0, 1, 6] = A
    assert PR.canonicalize(cmd, arg)["valid"].tolist() == [True]


def test_numericalize_rounds_half_to_even_and_clips_at_both_ends():
    vals = [1.5, 0.5, 2.5, 3.5, -0.5, -3.0, 254.5, 255.5, 17.49, 300.0]          # a clockwise path: rows stay in order
    want = [2.0, 0.0, 2.0, 4.0, 0.0, 0.0, 254.0, 255.0, 17.0, 255.0]
    seq = [(M, [vals[0], vals[1]]), (C, vals[2:8]), (L, vals[8:10])]
    cmd, arg = icon([seq])
    got = PR.canonicalize(cmd, arg, numericalize=256)
    assert got["args"][0, 0, 1, 9:].tolist() == want[0:2] and got["args"][0, 0, 2, 5:].tolist() == want[2:8]
    assert got["args"][0, 0, 3, 9:].tolist() == want[8:10]
    assert (got["args"][0, 0, :, :5] == -1).all() and (got["args"][0, 0, 1, :9] == -1).all()
    # the decisions are taken on the raw values: 17.49 -> 17 makes nothing degenerate after the fact, and n is the clip
    assert PR.canonicalize(cmd, arg, numericalize=4)["args"].max() == 3
    # the elementwise step on its own: the restatement and paths.numericalize (torch, any device)
    alone = PR.numericalize(arg, cmd, 256)
    assert np.array_equal(alone, got["args"])
    t = paths.numericalize(torch.from_numpy(arg), torch.from_numpy(cmd), 256)
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), alone)
    ai = torch.tensor([[[-1] * 9 + [-7, 300]]]), torch.tensor([[L]])
    assert paths.numericalize(*ai).tolist() == [[[-1] * 9 + [0, 255]]] and paths.numericalize(*ai).dtype == torch.int64
    z = torch.full((1, 1, 11), -1.0), torch.tensor([[Z]])
    assert paths.numericalize(*z).eq(-1).all()


def test_source_group_and_reversed_against_a_brute_force_reading():
    """one open sub-path per input group, every group in an x band of its own: an output group's points are the points of
    exactly one input group, in its order or in the opposite one"""
    rng = np.random.default_rng(5)
    for _ in range(40):
        G = int(rng.integers(1, 6))
        groups = []
        for g in range(G):
            n = int(rng.integers(2, 6))
            pts = np.stack([rng.permutation(40)[:n] + 50 * g, rng.permutation(250)[:n]], 1).astype(np.float32)
            groups.append([(M, pts[0])] + [(L, p) for p in pts[1:]])
        cmd, arg = icon(groups, G=G, S=8)
        got = PR.canonicalize(cmd, arg)
        assert got["n_groups"][0] == G and sorted(got["source_group"][0].tolist()) == list(range(G))
        for k in range(G):
            n = got["len_groups"][0, k]
            pts = got["args"][0, k, 1:1 + n, 9:].tolist()
            src = [g for g in range(G) if all(50 * g <= p[0] < 50 * g + 40 for p in pts)]
            assert src == [got["source_group"][0, k]]
            orig = [list(map(float, v)) for _, v in groups[src[0]]]
            assert pts == (orig[::-1] if got["reversed"][0, k] else orig)
            assert len(orig) == n


def test_random_float_icons_are_almost_all_decisive():
    """the condition tests/test_paths_gpu.py relies on, checked where only the restatement runs"""
    cmd, arg = PR.random_float_icons(200, seed=3)
    share = 1.0 - PR.decisive(cmd, arg).mean()
    assert share <= 0.05, share


class _FakeOps:
    def __init__(self):
        self.calls = []

    def canonicalize(self, commands, args, g_out, s_out, concat=False, numericalize=0):
        self.calls.append((commands, args, g_out, s_out, concat, numericalize))
        return {"commands": commands}


@pytest.fixture
def fake_ops(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(paths.ops, "canonicalize", fake.canonicalize)
    return fake


def test_canonicalize_checks_its_arguments(fake_ops):
    c3, a3 = torch.zeros(2, 8, 32), torch.zeros(2, 8, 32, 11)
    for bad in [(c3, a3[:, :, :31]), (c3, a3[..., :10]), (c3[0, 0], a3[0, 0]), (c3[None], a3[None]), (c3, a3[:1])]:
        with pytest.raises(ValueError):
            paths.canonicalize(*bad)
    with pytest.raises(ValueError, match="layout"):
        paths.canonicalize(c3, a3, layout="flat")
    with pytest.raises(ValueError, match="max_num_groups"):
        paths.canonicalize(c3[:, 0], a3[:, 0])
    with pytest.raises(ValueError, match="2048"):
        paths.canonicalize(torch.zeros(1, 8, 257), torch.zeros(1, 8, 257, 11))
    with pytest.raises(ValueError, match="2048"):
        paths.canonicalize(torch.zeros(1, 2049), torch.zeros(1, 2049, 11), max_num_groups=8)
    assert not fake_ops.calls
    paths.canonicalize(torch.zeros(1, 8, 256), torch.zeros(1, 8, 256, 11))
    assert fake_ops.calls.pop()[2:] == (8, 256, False, 0)


def test_canonicalize_shapes_dtypes_and_defaults(fake_ops):
    c3, a3 = torch.zeros(2, 8, 32), torch.zeros(2, 8, 32, 11, requires_grad=True)
    paths.canonicalize(c3, a3)
    c, a, g_out, s_out, concat, num = fake_ops.calls.pop()
    assert (g_out, s_out, concat, num) == (8, 32, False, 0) and c.shape == (2, 8, 32) and not a.requires_grad
    paths.canonicalize(c3, a3, max_num_groups=12, max_seq_len=40, layout="concat", numericalize=256)
    assert fake_ops.calls.pop()[2:] == (12, 42, True, 256)
    paths.canonicalize(c3[:, 0], a3[:, 0], max_num_groups=5)                       # (N, S): read as G = 1
    c, a, g_out, s_out, concat, num = fake_ops.calls.pop()
    assert c.shape == (2, 1, 32) and a.shape == (2, 1, 32, 11) and (g_out, s_out) == (5, 32) and c.is_contiguous()
    paths.canonicalize(c3.long(), a3.detach().long())
    assert fake_ops.calls.pop()[0].dtype == torch.int64
    for c, a in [(c3.long(), a3), (c3.half(), a3.half()), (c3.int(), a3.int())]:       # anything else is read as float32
        paths.canonicalize(c, a)
        c, a = fake_ops.calls.pop()[:2]
        assert c.dtype == a.dtype == torch.float32


def test_package_and_binding_declare_the_op():
    assert deepsvg_amd.paths is paths and "paths" in deepsvg_amd.__all__
    assert lib.ABI_VERSION == 19 and len(lib.SIGNATURES["dsvg_canonicalize"][1]) == 18
    assert (lib.DSVG_PATHS_GROUPED, lib.DSVG_PATHS_CONCAT) == (0, 1)
