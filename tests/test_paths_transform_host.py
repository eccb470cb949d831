"""deepsvg_amd.paths.transform and the float32 PackedSVGStore without a GPU: the restatement (tests/paths_transform_ref.py)
against the reference's own results (tests/golden/paths/transform.npz), the rules of the definition on hand-made rows, and the
Python surface against a fake `ops` that runs the restatement on what the wrappers hand to the kernel."""
import types

import numpy as np
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import dataset as D
from deepsvg_amd import lib, paths, svg_dataset
from deepsvg_amd.lib import DsvgError
from tests import paths_transform_ref as R

F = np.float32


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def padded(rows, S=None):
    """one group of [command, 11 arguments] rows -> commands (1, 1, S), args (1, 1, S, 11): SOS, rows, EOS..."""
    S = S or len(rows) + 2
    cmd = np.full((1, 1, S), R.EOS, dtype=F)
    args = np.full((1, 1, S, 11), -1.0, dtype=F)
    cmd[0, 0, 0] = R.SOS
    for i, r in enumerate(rows):
        cmd[0, 0, 1 + i], args[0, 0, 1 + i] = r[0], r[1:]
    return cmd, args


def line(x, y, c=R.L):
    return [c] + [-1.0] * 9 + [x, y]


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_on_every_golden_chain(gold):
    chains = R.golden_chains(gold)
    assert set(chains) >= {"a", "b", "c", "c_mean", "plain", "d0", "d1"} and 90.0 in gold["angles"]
    assert gold["commands"].shape == (30, 4, 16) and gold["cfg"].tolist() == [4, 14, 40]
    for tag, (steps, num) in chains.items():
        got = R.transform(gold["commands"], gold["args"], steps, num)
        assert got.dtype == F and np.array_equal(got, gold[f"{tag}/args"]), tag


def test_ties_round_half_to_even_after_a_translate_by_a_half():
    cmd, args = padded([line(2.0, 3.0, R.M), line(0.0, 1.0), line(254.0, 255.0)])
    out = R.transform(cmd, args, [("translate", (0.5, 0.5))], 256)[0, 0, 1:4, 9:]
    assert out.tolist() == [[2.0, 4.0], [0.0, 2.0], [254.0, 255.0]]             # 2.5 -> 2, 3.5 -> 4, 0.5 -> 0, 1.5 -> 2, 254.5 -> 254


def test_values_clip_at_both_ends_after_a_zoom_by_three():
    cmd, args = padded([line(10.0, 250.0, R.M), [R.C, -1, -1, -1, -1, -1, 0.0, 128.0, 255.0, 90.0, 170.0, 86.0]])
    out = R.transform(cmd, args, R.zoom_steps(3.0, 256), 256)[0, 0, 1:3]
    assert out[0, 9:].tolist() == [0.0, 255.0]                                  # -226 and 494
    assert out[1, 5:].tolist() == [0.0, 128.0, 255.0, 14.0, 254.0, 2.0]
    assert np.array_equal(out[0, :9], args[0, 0, 1, :9])                        # slots the mask does not enable: copied


def test_no_step_is_elided_a_scale_by_one_between_two_translates_is_not_the_identity():
    x = F(0.1)
    cmd, args = padded([line(x, x, R.M)])
    out = R.transform(cmd, args, R.zoom_steps(1.0, 256))[0, 0, 1, 9]
    assert out == (x - F(128)) + F(128) and out != x


def test_arc_rows_follow_their_rule():
    arc = [R.A, 3.0, 5.0, 30.0, 1.0, 0.0, -1, -1, -1, -1, 20.0, 40.0]
    cmd, args = padded([line(1.0, 2.0, R.M), arc])
    steps = [("translate", (7.0, -3.0)), ("scale", 1.5), ("rotate", 90.0), ("translate", (0.25, 0.25))]
    out = R.transform(cmd, args, steps)[0, 0, 2]
    c, s = F(np.cos(np.deg2rad(90.0))), F(np.sin(np.deg2rad(90.0)))
    x, y = F(27.0) * F(1.5), F(37.0) * F(1.5)
    assert out[9] == (c * x - s * y) + F(0.25) and out[10] == (s * x + c * y) + F(0.25)
    assert out[:5].tolist() == [4.5, 7.5, 120.0, 1.0, 0.0]                      # radii: scale only; phi + deg; flags copied
    assert out[5:9].tolist() == [-1.0] * 4
    num = R.transform(cmd, args, [("scale", 1.5)], 8)[0, 0, 2]
    assert num[:5].tolist() == [4.0, 7.0, 7.0, 1.0, 0.0] and num[9:].tolist() == [7.0, 7.0]     # 4.5 -> 4, 7.5 -> 8 -> clip 7


def test_rows_behind_the_first_eos_and_frame_rows_are_untouched():
    cmd, args = padded([line(1.0, 2.0, R.M), line(3.0, 4.0)], S=8)
    cmd[0, 0, 5], args[0, 0, 5] = R.L, line(9.0, 9.0)[1:]                      # a stale row behind the EOS
    cmd[0, 0, 6], args[0, 0, 6, 9:] = R.Z, (5.0, 5.0)
    args[0, 0, 0, 9:] = (6.0, 6.0)                                              # the SOS frame: live, nothing enabled
    out = R.transform(cmd, args, [("translate", (1.0, 1.0))], 256)
    assert out[0, 0, 1:3, 9:].tolist() == [[2.0, 3.0], [4.0, 5.0]]
    keep = [0, 3, 4, 5, 6, 7]
    assert np.array_equal(out[0, 0, keep], args[0, 0, keep])
    one = R.transform(cmd[:, 0], args[:, 0], [("translate", (1.0, 1.0))], 256)  # (N, S): the one-stage form
    assert np.array_equal(one, out[:, 0])


# ---- the Python surface, against a fake ops that runs the restatement ---------------------------------------------------
class _FakeOps:
    STEP_KINDS = {"translate": 0, "scale": 1, "rotate": 2}

    def __init__(self):
        self.calls = []

    def paths_transform(self, commands, args, kinds, params, numericalize=0):
        self.calls.append((commands, args, list(kinds), params, numericalize))
        assert commands.dim() == 3 and commands.dtype == args.dtype == params.dtype == torch.float32
        assert commands.is_contiguous() and args.is_contiguous() and params.is_contiguous() and not args.requires_grad
        return torch.from_numpy(R.transform_packed(commands.numpy(), args.numpy(), kinds, params.numpy(), numericalize))


@pytest.fixture
def fake_ops(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(paths, "ops", fake)
    return fake


def test_wrappers_build_the_reference_s_step_lists(gold, fake_ops):
    cmd, args = torch.from_numpy(gold["commands"]), torch.from_numpy(gold["args"]).requires_grad_()
    f, vec = torch.from_numpy(gold["draws"][:, 2]), torch.from_numpy(gold["draws"][:, :2])
    a = paths.normalize(cmd, args, (32, 20), target=24)
    a = paths.zoom(a["commands"], a["args"], 0.9, viewbox=24)
    assert np.array_equal(a["args"].numpy(), gold["a/args"]) and len(fake_ops.calls) == 2
    b = paths.augment(cmd, args, f, vec, viewbox=24)
    assert np.array_equal(b["args"].numpy(), gold["b/args"]) and fake_ops.calls[-1][2] == [0, 1, 0, 0]
    c = paths.augment(cmd, args, f, vec, viewbox=24, numericalize=256)
    assert np.array_equal(c["args"].numpy(), gold["c/args"])
    assert fake_ops.calls[-1][2] == [0, 1, 0, 0, 0, 1, 0] and fake_ops.calls[-1][4] == 256      # one launch, K = 7
    m = paths.augment(cmd, args, *paths.augment_params(30, mean=True, device="cpu"), viewbox=24, numericalize=256)
    assert np.array_equal(m["args"].numpy(), gold["c_mean/args"])
    for j, deg in enumerate(gold["angles"]):
        r = paths.rotate(cmd, args, float(deg), viewbox=24)
        assert np.array_equal(r["args"].numpy(), gold[f"d{j}/args"]), deg
    t = paths.translate(cmd[:, 0], args[:, 0], (1.5, -2.0))                    # (N, S)
    assert t["args"].shape == (30, 16, 11) and t["commands"].shape == (30, 16) and fake_ops.calls[-1][0].shape == (30, 1, 16)
    assert np.array_equal(t["args"].numpy(), R.transform(gold["commands"][:, 0], gold["args"][:, 0], [("translate", (1.5, -2.0))]))
    z = paths.zoom(cmd, args, f, center=vec, viewbox=(32, 20))                 # per-item factor and centre
    assert np.array_equal(z["args"].numpy(), R.transform(gold["commands"], gold["args"], R.zoom_steps(f.numpy(), (32, 20), vec.numpy())))
    deg = torch.linspace(-170.0, 170.0, 30)
    r = paths.rotate(cmd, args, deg, viewbox=24)
    assert np.array_equal(r["args"].numpy(), R.transform(gold["commands"], gold["args"], R.rotate_steps(deg.numpy(), 24)))


def test_every_public_function_checks_its_arguments(fake_ops):
    c3, a3 = torch.zeros(2, 4, 8), torch.zeros(2, 4, 8, 11)
    T = [("translate", (1, 2))]
    for bad in [(c3, a3[:, :, :7]), (c3, a3[..., :10]), (c3[0, 0], a3[0, 0]), (c3[None], a3[None]), (c3[:0], a3[:0]),
                (torch.zeros(1, 8, 257), torch.zeros(1, 8, 257, 11))]:
        with pytest.raises(ValueError):
            paths.transform(*bad, T)
    nan, inf = float("nan"), float("inf")
    for steps in [[], T * 17, [("shear", 1.0)], ["translate"], [("translate", 1.0, 2.0)], [("translate", (1, 2, 3))],
                  [("translate", (1, nan))], [("scale", inf)], [("scale", (1, 2))], [("rotate", nan)], [("rotate", "90")],
                  [("scale", True)], [("translate", torch.zeros(2))], [("translate", torch.zeros(3, 2))],
                  [("scale", torch.zeros(2, 1))], [("rotate", torch.zeros(3))], "translate", None]:
        with pytest.raises(ValueError):
            paths.transform(c3, a3, steps)
    for num in (0, -1, True):
        with pytest.raises(ValueError):
            paths.transform(c3, a3, T, numericalize=num)
    with pytest.raises(ValueError):
        paths.zoom(c3, a3, inf)
    with pytest.raises(ValueError):
        paths.zoom(c3, a3, 0.9, center=(1, 2, 3))
    with pytest.raises(ValueError):
        paths.zoom(c3, a3, 0.9, viewbox=(24, nan))
    with pytest.raises(ValueError):
        paths.rotate(c3, a3, inf)
    with pytest.raises(ValueError):
        paths.translate(c3, a3, 1.0 + 2j)
    with pytest.raises(ValueError):
        paths.normalize(c3, a3, 0)
    with pytest.raises(ValueError):
        paths.normalize(c3, a3, 24, target=nan)
    with pytest.raises(ValueError):
        paths.augment(c3, a3, 0.7, (0, 0, 0))
    with pytest.raises(ValueError):
        paths.augment(c3, a3, torch.zeros(3), (0, 0))
    with pytest.raises(ValueError):
        paths.augment(c3, a3, 0.7, (0, 0), numericalize=0)
    for bad in (0, 2.0, True):
        with pytest.raises(ValueError):
            paths.augment_params(bad, device="cpu")
    with pytest.raises(ValueError):
        paths.augment_params(4, viewbox=0, device="cpu")
    assert not fake_ops.calls
    paths.transform(c3, a3, T * 16, numericalize=256)                           # the limits themselves
    paths.transform(torch.zeros(1, 8, 256), torch.zeros(1, 8, 256, 11), T)
    assert len(fake_ops.calls) == 2 and fake_ops.calls[0][3].shape == (2, 16, 3)


def test_augment_params_ranges_and_mean():
    g = torch.Generator().manual_seed(5)
    f, v = paths.augment_params(4096, generator=g)
    assert f.shape == (4096,) and v.shape == (4096, 2) and f.dtype == v.dtype == torch.float32
    assert 0.6 <= float(f.min()) < 0.61 and 0.79 < float(f.max()) <= 0.8 + 1e-6
    lim = 2.5 * 256 / 24
    assert -lim <= float(v.min()) < -0.98 * lim and 0.98 * lim < float(v.max()) <= lim
    assert abs(float(f.mean()) - 0.7) < 0.01 and abs(float(v.mean())) < 0.05 * lim
    f24, v24 = paths.augment_params(4096, viewbox=24, generator=torch.Generator().manual_seed(5))
    assert torch.equal(f24, f) and float(v24.abs().max()) <= 2.5
    f, v = paths.augment_params(3, mean=True, device="cpu")
    assert f.tolist() == [float(F(0.7))] * 3 and v.tolist() == [[0.0, 0.0]] * 3


def test_package_and_binding_declare_the_ops():
    assert set(paths.__all__) >= {"transform", "zoom", "rotate", "translate", "normalize", "augment", "augment_params"}
    assert deepsvg_amd.paths is paths
    assert lib.ABI_VERSION == 19
    assert len(lib.SIGNATURES["dsvg_paths_transform"][1]) == 11 and len(lib.SIGNATURES["dsvg_assemble_augmented"][1]) == 19
    assert (lib.DSVG_STEP_TRANSLATE, lib.DSVG_STEP_SCALE, lib.DSVG_STEP_ROTATE, lib.DSVG_MAX_STEPS) == (0, 1, 2, 16)
    assert "SVG.numericalize" in paths.__doc__ and "svg_dataset.SVGDataset.batch" in paths.__doc__


# ---- the float32 store ---------------------------------------------------------------------------------------------------
def _icons(gold):
    return [[[R.rows14(g) for g in R.groups_of(c, a) if len(g)]] for c, a in zip(gold["commands"], gold["args"])]


def test_float_store_round_trip(gold, tmp_path):
    icons = _icons(gold)
    st = D.PackedSVGStore.from_icons(icons, labels=list(range(30)), max_num_groups=4, numericalized=False, viewbox=24.0)
    assert st.rows.dtype == np.float32 and st.rows.shape[1] == 12 and st.is_float and st.viewbox == 24.0 and not st.is_device
    assert st.slot_off.shape == (30 * 4 + 1,) and st.max_group_len == 14 and st.max_total_len <= 40
    for i, (variant,) in enumerate(icons):
        for g in range(4):
            lo, hi = st.slot_off[i * 4 + g], st.slot_off[i * 4 + g + 1]
            want = variant[g][:, list(D.ROW_COLS)] if g < len(variant) else np.zeros((0, 12), F)
            assert np.array_equal(st.rows[lo:hi], want)
    st.save(tmp_path / "svg_store.npz")
    st2 = D.PackedSVGStore.load(tmp_path / "svg_store.npz")
    for name in ("rows", "slot_off", "var_base", "filling", "label"):
        assert np.array_equal(getattr(st, name), getattr(st2, name)) and getattr(st, name).dtype == getattr(st2, name).dtype
    assert st2.viewbox == 24.0 and st2.is_float and (st2.G, st2.max_group_len) == (4, 14)
    # the int16 form keeps no view box through save / load
    it = D.PackedSVGStore.from_icons([[[np.zeros((2, 14), F)]]], max_num_groups=4)
    it.save(tmp_path / "int.npz")
    assert D.PackedSVGStore.load(tmp_path / "int.npz").viewbox is None and not it.is_float
    # both data sets need the device, and each refuses the other's store
    cfg = types.SimpleNamespace(data_dir=str(tmp_path), model_args=["commands"], max_num_groups=4, max_seq_len=14,
                                max_total_len=40, device="cpu")
    with pytest.raises(DsvgError, match="HIP device"):
        svg_dataset.load_dataset(cfg)
    with pytest.raises(DsvgError, match="float32"):
        D.SVGTensorDataset(store=st, model_args=["commands"], max_num_groups=4, max_seq_len=14)
    with pytest.raises(DsvgError, match="float32"):
        svg_dataset.SVGDataset(store=it, model_args=["commands"], max_num_groups=4, max_seq_len=14)
    with pytest.raises(DsvgError, match="max_seq_len"):
        svg_dataset.SVGDataset(store=st, model_args=["commands"], max_num_groups=4, max_seq_len=13, device="cpu")


def test_from_batch_equals_a_plain_gather(gold):
    cmd, args = torch.from_numpy(gold["commands"]), torch.from_numpy(gold["args"])
    lens = ((cmd < R.EOS).sum(-1)).to(torch.int32)
    fill = torch.arange(120).reshape(30, 4) % 3
    st = D.PackedSVGStore.from_batch(cmd, args, lens, filling=fill, labels=torch.arange(30), viewbox=24.0)
    want = D.PackedSVGStore.from_icons(_icons(gold), max_num_groups=4, numericalized=False, viewbox=24.0)
    assert st.rows.dtype == torch.float32 and st.slot_off.dtype == torch.int32 and st.var_base.dtype == torch.int32
    assert np.array_equal(st.rows.numpy(), want.rows) and np.array_equal(st.slot_off.numpy(), want.slot_off)
    assert np.array_equal(st.var_base.numpy(), want.var_base) and torch.equal(st.filling, fill) and st.label.tolist() == list(range(30))
    assert (st.max_group_len, st.max_total_len, st.viewbox, st.G) == (want.max_group_len, want.max_total_len, 24.0, 4)
    empty = D.PackedSVGStore.from_batch(cmd[:2], args[:2], torch.zeros(2, 4, dtype=torch.int32))
    assert empty.rows.shape == (1, 12) and empty.slot_off.tolist() == [0] * 9 and empty.viewbox == 256.0
    with pytest.raises(DsvgError):
        D.PackedSVGStore.from_batch(cmd, args[:, :, :15], lens)


def test_the_integer_default_still_refuses_non_integers():
    t = np.zeros((3, 14), F)
    t[1, 12] = 0.5
    with pytest.raises(DsvgError, match="numericalised"):
        D.PackedSVGStore.from_icons([[[t]]], max_num_groups=8)
    st = D.PackedSVGStore.from_icons([[[t]]], max_num_groups=8, numericalized=False)
    assert st.rows[1, 10] == 0.5 and st.viewbox == 24.0
    bad = t.copy()
    bad[2, 0] = 2.5
    with pytest.raises(DsvgError, match="command"):
        D.PackedSVGStore.from_icons([[[bad]]], max_num_groups=8, numericalized=False)
    bad = t.copy()
    bad[2, 13] = np.inf
    with pytest.raises(DsvgError, match="finite"):
        D.PackedSVGStore.from_icons([[[bad]]], max_num_groups=8, numericalized=False)
    with pytest.raises(DsvgError, match="viewbox"):
        D.PackedSVGStore.from_icons([[[t]]], max_num_groups=8, numericalized=False, viewbox=0)
