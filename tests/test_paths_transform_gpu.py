"""dsvg_paths_transform on the GPU against the restatement (tests/paths_transform_ref.py) and the reference's own results
(tests/golden/paths/transform.npz), everything by equality."""
import numpy as np
import pytest
import torch

from deepsvg_amd import paths
from tests import paths_transform_ref as R
from tests.poison import three_runs

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def random_padded(rng, shape):
    """padded icons of every kind of row: m / l / c / a / z rows with float coordinates, groups that are empty, full to the
    last row (no EOS at all) and anything between, and stale rows of any command behind the first EOS"""
    S = shape[-1]
    cmd = rng.choice([R.M, R.L, R.C, R.A, R.Z, R.SOS, R.EOS], size=shape, p=[.1, .25, .3, .15, .05, .05, .1]).astype(F)
    args = rng.uniform(0, 256, size=shape + (11,)).astype(F)
    flat = cmd.reshape(-1, S)
    flat[:, 0] = R.SOS
    lens = rng.integers(0, S + 1, size=len(flat))
    lens[:3] = (0, S - 1, S)
    for row, n in zip(flat, lens):
        live = row[1:1 + n]
        live[live == R.EOS] = R.L
        if 1 + n < S:
            row[1 + n] = R.EOS
    unused = ~R.CMD_ARGS_MASK[cmd.astype(np.int64)]
    args[unused & (rng.uniform(size=unused.shape) < 0.8)] = -1.0
    return cmd, args


def steps_for(K, n, rng):
    t = lambda: rng.uniform(-40, 40, size=(n, 2)).astype(F)
    f = lambda: rng.uniform(0.5, 1.5, size=n).astype(F)
    d = lambda: rng.uniform(-180, 180, size=n).astype(F)
    if K == 1:
        return [("translate", t())], 0
    if K == 7:
        return R.augment_steps(rng.uniform(0.6, 0.8, size=n).astype(F), t(), 256, 256), 256
    steps = []
    for k in range(16):
        steps.append([("translate", t()), ("scale", f()), ("rotate", d()), ("translate", (0.5, -1.25)), ("scale", 1.0),
                      ("rotate", 90.0)][k % 6])
    return steps, 0


def on_device(steps, device):
    """the restatement's step lists as the wrappers take them: one value per item -> a device tensor, constants -> numbers"""
    out = []
    for kind, v in steps:
        if isinstance(v, np.ndarray) and v.shape != (2,):
            v = torch.from_numpy(np.ascontiguousarray(v)).to(device)
        elif isinstance(v, np.ndarray):
            v = (float(v[0]), float(v[1]))
        elif isinstance(v, np.floating):
            v = float(v)
        out.append((kind, v))
    return out


@pytest.mark.parametrize("shape", [(3, 4, 80), (1, 8, 256), (5, 50)], ids=str)
@pytest.mark.parametrize("K", [1, 7, 16])
def test_transform_equals_the_restatement(gpu_device, shape, K):
    rng = np.random.default_rng(100 * K + len(shape))
    cmd, args = random_padded(rng, shape)
    steps, num = steps_for(K, shape[0], rng)
    assert len(steps) == K
    want = R.transform(cmd, args, steps, num)
    out = paths.transform(torch.from_numpy(cmd).to(gpu_device), torch.from_numpy(args).to(gpu_device),
                          on_device(steps, gpu_device), numericalize=num or None)
    got = out["args"].cpu().numpy()
    assert got.shape == args.shape and got.dtype == F and np.array_equal(out["commands"].cpu().numpy(), cmd)
    assert np.array_equal(got, want, equal_nan=True)
    assert not np.array_equal(got, args)                                      # and it did something


def test_golden_icons_through_every_stored_chain(gpu_device, gold):
    cmd, args = torch.from_numpy(gold["commands"]).to(gpu_device), torch.from_numpy(gold["args"]).to(gpu_device)
    f = torch.from_numpy(gold["draws"][:, 2]).to(gpu_device)
    vec = torch.from_numpy(gold["draws"][:, :2]).to(gpu_device)
    eq = lambda res, tag: np.array_equal(res["args"].cpu().numpy(), gold[f"{tag}/args"])
    a = paths.normalize(cmd, args, (32, 20), target=24)
    assert eq(paths.zoom(a["commands"], a["args"], 0.9, viewbox=24), "a")
    assert eq(paths.augment(cmd, args, f, vec, viewbox=24), "b")
    assert eq(paths.augment(cmd, args, f, vec, viewbox=24, numericalize=256), "c")
    assert eq(paths.augment(cmd, args, *paths.augment_params(30, mean=True, device=gpu_device), viewbox=24, numericalize=256),
              "c_mean")
    plain = paths.normalize(cmd, args, 24, target=256)
    assert np.array_equal(paths.numericalize(plain["args"], cmd).cpu().numpy(), gold["plain/args"])
    for j, deg in enumerate(gold["angles"]):
        assert eq(paths.rotate(cmd, args, float(deg), viewbox=24), f"d{j}"), deg
    # every chain once more from the restatement's step lists, per-item tensors where the chain has them
    for tag, (steps, num) in R.golden_chains(gold).items():
        steps = [(k, np.asarray(v, dtype=F) if isinstance(v, np.ndarray) else v) for k, v in steps]
        assert eq(paths.transform(cmd, args, on_device(steps, gpu_device), numericalize=num or None), tag), tag


def test_draws_stay_on_the_device_and_follow_the_generator(gpu_device):
    g = torch.Generator(device=gpu_device).manual_seed(11)
    f, v = paths.augment_params(2048, viewbox=24, generator=g)
    assert f.device.type == "cuda" and v.shape == (2048, 2)
    assert 0.6 <= float(f.min()) and float(f.max()) <= 0.8 + 1e-6 and float(v.abs().max()) <= 2.5
    f2, v2 = paths.augment_params(2048, viewbox=24, generator=torch.Generator(device=gpu_device).manual_seed(11))
    assert torch.equal(f, f2) and torch.equal(v, v2)


def test_no_result_depends_on_uninitialised_memory(gpu_device):
    rng = np.random.default_rng(7)
    cmd, args = random_padded(rng, (3, 4, 80))
    steps, num = steps_for(7, 3, rng)
    cmd_d, args_d = torch.from_numpy(cmd).to(gpu_device), torch.from_numpy(args).to(gpu_device)
    runs = three_runs(lambda: paths.transform(cmd_d, args_d, on_device(steps, gpu_device), numericalize=num)["args"])
    want = torch.from_numpy(R.transform(cmd, args, steps, num)).to(gpu_device)
    for r in runs:
        assert torch.equal(r, want)
