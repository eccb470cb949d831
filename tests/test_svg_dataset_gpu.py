"""deepsvg_amd.svg_dataset.SVGDataset (dsvg_assemble_augmented) on the GPU, by equality three ways: against what the
reference's `preprocess` + `get_data` return (tests/golden/paths/transform.npz), against the restatement's rows packed into a
numericalised int16 store and assembled by the existing SVGTensorDataset (the two assembly kernels share the token layout), and
against itself after the same seed."""
import types

import numpy as np
import pytest
import torch

from deepsvg_amd import dataset as D
from deepsvg_amd import paths, svg_dataset
from tests import paths_transform_ref as R
from tests.poison import three_runs

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ["commands", "args", "args_rel", "commands_grouped", "args_grouped", "args_rel_grouped"]
VB = 24.0


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def group(rng, n):
    """n rows [command, 11 arguments]: an `m`, then `l` / `c`, float coordinates in the view box"""
    g = np.full((n, 12), -1.0, dtype=F)
    if n:
        g[:, 0] = rng.integers(1, 3, size=n)
        g[0, 0] = R.M
        for r in g:
            k = 6 if r[0] == R.C else 2
            r[12 - k:] = rng.uniform(0, VB, size=k)
    return g


def icons_for(rng, G, S, T):
    """12 icons: one with no rows, one with an empty last group, one with a group of exactly S rows, one with an empty group
    between two others, and seeded ones"""
    icons = [[], [group(rng, 3), group(rng, 2), group(rng, 0)], [group(rng, S), group(rng, 1)],
             [group(rng, 2), group(rng, 0), group(rng, 4)]]
    while len(icons) < 12:
        lens, left = [], T
        for _ in range(int(rng.integers(1, G + 1))):
            lens.append(int(rng.integers(0, min(S, left) + 1)))
            left -= lens[-1]
        icons.append([group(rng, n) for n in lens])
    return icons


def float_dataset(icons, G, S, T, device, keys=KEYS, **kw):
    st = D.PackedSVGStore.from_icons([[[R.rows14(g) for g in groups]] for groups in icons], labels=list(range(len(icons))),
                                     max_num_groups=G, numericalized=False, viewbox=VB)
    return svg_dataset.SVGDataset(store=st, model_args=keys, max_num_groups=G, max_seq_len=S, max_total_len=T, device=device, **kw)


def steps_of(aug):
    """one item's chain: (dx, dy, factor), or None for preprocess(augment=False)"""
    return R.normalize_steps(VB, 256) if aug is None else R.augment_steps(F(aug[2]), (F(aug[0]), F(aug[1])), VB, 256)


def via_int16_store(icons, idx, augs, G, S, T, device, keys=KEYS):
    """the restatement's transformed and rounded rows of every ITEM, packed as a numericalised store of their own and assembled
    by the int16 kernel"""
    items = [[R.rows14(np.concatenate([g[:, :1], rows], axis=1)) for g, rows in
              zip(icons[i], R.store_rows(icons[i], steps_of(a), 256))] for i, a in zip(idx, augs)]
    st = D.PackedSVGStore.from_icons([[groups] for groups in items], max_num_groups=G)
    ds = D.SVGTensorDataset(store=st, model_args=keys, max_num_groups=G, max_seq_len=S, max_total_len=T, device=device)
    return ds.batch(list(range(len(items))), random_aug=False)


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("cfg", [(4, 14, 40), (8, 30, 50)], ids=str)
def test_batches_equal_the_restatement_through_the_int16_kernel(gpu_device, cfg):
    G, S, T = cfg
    rng = np.random.default_rng(G)
    icons = icons_for(rng, G, S, T)
    ds = float_dataset(icons, G, S, T, gpu_device)
    assert len(ds) == 12 and ds.store.rows.dtype == torch.float32 and ds.store.viewbox == VB
    # every icon, pinned draws that differ between items
    idx = list(range(12))
    augs = np.concatenate([rng.uniform(-2.5, 2.5, size=(12, 2)), rng.uniform(0.6, 0.8, size=(12, 1))], axis=1).astype(F)
    out = ds.batch(idx, aug=torch.from_numpy(augs))
    want = via_int16_store(icons, idx, augs, G, S, T, gpu_device)
    same(out, want)
    assert out["commands"].shape == (12, G, S + 2) and out["args_rel_grouped"].shape == (12, 1, T + 2, 11)
    assert out["commands"][0, :, 1].eq(R.EOS).all() and out["commands"][2, 0, S].lt(R.EOS) and out["commands"][2, 0, S + 1] == R.EOS
    # the same icon several times in one batch with different draws: parameters belong to items, not to icons
    idx = [2, 2, 5, 2, 1, 1]
    augs = np.array([[0, 0, 0.7], [2.5, -2.5, 0.6], [1, 1, 0.8], [-1.25, 0.5, 0.75], [0, 0, 0.7], [0.125, 0, 0.7]], dtype=F)
    out = ds.batch(idx, aug=torch.from_numpy(augs).to(gpu_device))
    same(out, via_int16_store(icons, idx, augs, G, S, T, gpu_device))
    assert not torch.equal(out["args"][0], out["args"][1]) and not torch.equal(out["args"][4], out["args"][5])
    # preprocess(augment=False), a subset of the keys (the grouped layout alone), and the per-item surface
    out = ds.batch([3, 0, 11], ["args_rel_grouped", "commands_grouped", "label"], random_aug=False)
    want = via_int16_store(icons, [3, 0, 11], [None] * 3, G, S, T, gpu_device, ["args_rel_grouped", "commands_grouped"])
    assert out.pop("label").tolist() == [3, 0, 11]
    same(out, want)
    item = ds.get(12 + 3, ["args_rel"], random_aug=False)                      # idx % n_icons
    assert torch.equal(item["args_rel"], via_int16_store(icons, [3], [None], G, S, T, gpu_device, ["args_rel"])["args_rel"][0])
    # args_rel: the first real command of a sequence keeps its position, every other is relative to the one before it
    full = ds.batch([3], random_aug=False)
    a, r = full["args"][0], full["args_rel"][0]
    assert torch.equal(r[0, 1, 9:], a[0, 1, 9:] + 255) and torch.equal(r[0, 2, 9:], a[0, 2, 9:] - a[0, 1, 9:] + 255)
    ag, rg = full["args_grouped"][0, 0], full["args_rel_grouped"][0, 0]
    assert torch.equal(rg[3, 9:], ag[3, 9:] - ag[2, 9:] + 255)                  # across the group boundary (and the empty group)


def test_batches_equal_the_reference_s_get_data(gpu_device, gold):
    G, S, T = gold["cfg"].tolist()
    icons = [[g for g in R.groups_of(c, a) if len(g)] for c, a in zip(gold["commands"], gold["args"])]
    ds = float_dataset(icons, G, S, T, gpu_device)
    n = len(icons)
    draws = torch.from_numpy(gold["draws"].astype(F))
    mean = torch.tensor([[0.0, 0.0, 0.7]]).repeat(n, 1)
    for tag, kw in (("c", dict(aug=draws)), ("c_mean", dict(aug=mean)), ("plain", dict(random_aug=False))):
        out = ds.batch(list(range(n)), **kw)
        for k in KEYS:
            got = out[k].cpu().numpy()
            assert got.shape == gold[f"{tag}/{k}"].shape and np.array_equal(got, gold[f"{tag}/{k}"]), (tag, k)


def test_random_augmentation_is_seeded_per_item_and_drawn_on_the_device(gpu_device):
    G, S, T = 4, 14, 40
    icons = icons_for(np.random.default_rng(1), G, S, T)
    ds = float_dataset(icons, G, S, T, gpu_device, deferred=True)
    idx = [1, 2, 2, 3, 4, 5, 6, 7]
    a = ds.manual_seed(3).batch(idx)
    b = ds.manual_seed(3).batch(idx)
    c = ds.batch(idx)                                                           # the generator has moved on
    same(a, b)
    assert not torch.equal(a["args"], c["args"]) and not torch.equal(a["args"][1], a["args"][2])
    f, v = paths.augment_params(len(idx), viewbox=VB, generator=torch.Generator(device=gpu_device).manual_seed(3))
    same(a, ds.batch(idx, aug=torch.cat([v, f[:, None]], dim=1)))
    live = a["args"][a["args"] >= 0]
    assert live.numel() and bool((live == live.round()).all()) and float(live.max()) <= 255
    # the reference's loader seam: DataLoader(dataset, collate_fn=cfg.collate_fn) (deepsvg/train.py:27-28)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, drop_last=True, num_workers=0,
                                         collate_fn=D.device_collate)
    batches = list(loader)
    assert len(batches) == 3 and all(d["commands"].shape == (4, G, S + 2) and d["commands"].is_cuda for d in batches)
    assert all(d["args_rel_grouped"].shape == (4, 1, T + 2, 11) for d in batches)


def test_load_dataset_reads_a_saved_float_store(gpu_device, tmp_path):
    G, S, T = 4, 14, 40
    icons = icons_for(np.random.default_rng(2), G, S, T)
    ds = float_dataset(icons, G, S, T, gpu_device)
    ds.store.save(tmp_path / svg_dataset.STORE_FILE)
    cfg = types.SimpleNamespace(data_dir=str(tmp_path), model_args=KEYS, max_num_groups=G, max_seq_len=S, max_total_len=T,
                                collate_fn=D.device_collate, device=gpu_device)
    ds2 = svg_dataset.load_dataset(cfg)
    assert ds2.deferred and ds2.store.viewbox == VB and ds2.store.rows.dtype == torch.float32 and ds2.store.rows.is_cuda
    same(ds.batch(list(range(12)), random_aug=False), ds2.batch(list(range(12)), random_aug=False))
    # a store packed on the device from padded tensors gives the same batches
    padded = ds.batch(list(range(12)), ["commands", "args"], random_aug=False)
    lens = (padded["commands"] < R.EOS).sum(-1).to(torch.int32)
    st = D.PackedSVGStore.from_batch(padded["commands"], padded["args"], lens, viewbox=256.0)
    assert st.is_device and st.rows.dtype == torch.float32
    ds3 = svg_dataset.SVGDataset(store=st, model_args=KEYS, max_num_groups=G, max_seq_len=S, max_total_len=T)
    again = ds3.batch(list(range(12)), ["commands", "args"], random_aug=False)      # integers in the 256 box: a fixed point
    same(padded, again)


def test_no_batch_depends_on_uninitialised_memory(gpu_device):
    G, S, T = 4, 14, 40
    rng = np.random.default_rng(4)
    icons = icons_for(rng, G, S, T)
    ds = float_dataset(icons, G, S, T, gpu_device)
    idx = [0, 1, 2, 3, 2, 11]
    augs = np.concatenate([rng.uniform(-2.5, 2.5, size=(6, 2)), rng.uniform(0.6, 0.8, size=(6, 1))], axis=1).astype(F)
    aug = torch.from_numpy(augs).to(gpu_device)
    runs = three_runs(lambda: ds.batch(idx, aug=aug))
    want = via_int16_store(icons, idx, augs, G, S, T, gpu_device)
    for r in runs:
        same(r, want)
