"""tests/poison.py itself, on the host: what it patches, what it fills, `only` / `log`; that the product allocates through
nothing else; and that the Python layers of the model read no buffer they did not write (emulated ops, NaN poison)."""
import os
import re

import pytest
import torch

import deepsvg_amd
from deepsvg_amd.synthetic import make_batch
from oracle import svg_transformer_oracle as O
from tests import helpers as H
from tests.poison import poisoned_empty, three_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_patch_covers_both_constructors_and_is_undone():
    real = (torch.empty, torch.empty_like)
    with poisoned_empty(NAN):
        assert torch.empty is not real[0] and torch.empty_like is not real[1]
        assert torch.isnan(torch.empty(7, 3)).all()
        assert torch.isnan(torch.empty_like(torch.zeros(5))).all()
    assert (torch.empty, torch.empty_like) == real
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned_empty(NAN):
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like) == real
    with poisoned_empty(NAN):               # nests, and unwinds in order
        with poisoned_empty(0.0):
            assert torch.equal(torch.empty(4), torch.zeros(4))
        assert torch.isnan(torch.empty(4)).all()
    assert (torch.empty, torch.empty_like) == real


@pytest.mark.parametrize("fill", [NAN, 0.0, 3.5])
def test_fill_rules(fill):
    with poisoned_empty(fill):
        for dt in (torch.float32, torch.bfloat16):
            for t in (torch.empty(3, 5, dtype=dt), torch.empty((3, 5), dtype=dt, device="cpu"),
                      torch.empty_like(torch.ones(3, 5, dtype=dt)), torch.empty_like(torch.ones(3, 5), dtype=dt)):
                assert t.dtype == dt and t.shape == (3, 5)
                assert torch.isnan(t).all() if fill != fill else bool((t == fill).all())
        for dt in (torch.int32, torch.int64, torch.bool):           # never poisoned: always zero
            for t in (torch.empty(6, dtype=dt), torch.empty_like(torch.ones(6, dtype=dt)), torch.empty_like(torch.ones(6), dtype=dt)):
                assert t.dtype == dt and torch.count_nonzero(t) == 0
        assert torch.empty(0).numel() == 0
        leaf = torch.empty(4, requires_grad=True)
        assert leaf.requires_grad and leaf.is_leaf


def test_only_and_log():
    from deepsvg_amd import paths
    log = []
    with poisoned_empty(NAN, log=log):
        torch.empty(3)                                              # not inside the product: not logged
        assert log == []
        _alloc_in_product(paths)
    assert len(log) == 1 and log[0][0] == "deepsvg_amd/paths.py" and isinstance(log[0][1], int)
    with poisoned_empty(NAN, log=log):
        _alloc_in_product(paths)
    assert len(log) == 1                                            # each site once
    with poisoned_empty(NAN, only=log):
        assert torch.isnan(_alloc_in_product(paths)).all()
        assert torch.empty(3).shape == (3,)                         # another site: left alone (whatever it holds)
    with poisoned_empty(0.0, only=[("deepsvg_amd/paths.py", -1)]):
        real = torch.empty
        t = _alloc_in_product(paths)
        assert t.shape == (2, 2) and real is torch.empty


def _alloc_in_product(mod):
    """an allocation whose call stack passes through a frame of deepsvg_amd/ (code compiled under that module's file name)"""
    ns = {"torch": torch}
    exec(compile("\n" * 4 + "def alloc():\n    return torch.empty(2, 2)\n", mod.__file__, "exec"), ns)
    return ns["alloc"]()


def test_product_allocates_through_empty_and_empty_like_only():
    """poisoned_empty sees every uninitialised buffer of the product only as long as the product makes them with
    `torch.empty` / `torch.empty_like`, called by attribute"""
    other = re.compile(r"new_empty|empty_strided|empty_permuted|empty_quantized|resize_|resize_as_|\.new\(|\.set_\(|"
                       r"torch\.\w*Tensor\(|torch\.\w*Storage\(|from\s+torch\s+import|import\s+torch\s+as|"
                       r"=\s*torch\.empty(_like)?\s*($|[^(\w])|getattr\(torch")
    n_empty, bad = 0, []
    d = os.path.join(ROOT, "deepsvg_amd")
    for f in sorted(os.listdir(d)):
        if not f.endswith(".py"):
            continue
        for i, line in enumerate(open(os.path.join(d, f)), 1):
            code = line.split("#", 1)[0]
            n_empty += len(re.findall(r"\btorch\.empty(?:_like)?\(", code))
            if other.search(code):
                bad.append(f"{f}:{i}: {line.strip()}")
            # every other spelling of `empty` must be one of the two calls by attribute
            for m in re.finditer(r"\bempty\w*\s*\(", code):
                if not re.search(r"torch\.empty(_like)?\s*\($", code[:m.end()]):
                    bad.append(f"{f}:{i}: {line.strip()}")
    assert not bad, "\n".join(bad)
    assert n_empty > 150                                            # the scan found the product's allocations


def _emulated_run(kind, n, seed, dtype=torch.float32, train=False):
    cfg = H.build_cfg(kind)
    commands, args = make_batch(n, seed=seed)
    torch.manual_seed(3)
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(H.weights_for(deepsvg_amd.SVGTransformer(cfg), 7))
    model.set_compute_dtype(dtype)
    model.train(train)
    model.zero_grad()
    out = model(commands, args, commands, args, params={})
    ld = deepsvg_amd.SVGLoss(cfg)(out, None, weights=O.DEFAULT_WEIGHTS)
    ld["loss"].backward()
    outs = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
    grads = {n_: p.grad.detach().clone() for n_, p in model.named_parameters() if p.grad is not None}
    return {k: float(v.detach()) for k, v in ld.items()}, outs, grads


@pytest.mark.parametrize("kind", ["hier", "hier_vae"])
def test_python_layers_read_no_empty_buffer(kind, emulated_ops):
    """forward + loss + backward on the plain-torch restatements of every op: the layers above the kernels (model.py,
    functional.py, loss.py, the workspaces) hand no buffer on that they did not fill"""
    import deepsvg_amd.model as M
    orig = M.torch.randn_like
    gen = torch.Generator().manual_seed(0)
    eps = {}

    def randn_like(t):                                  # the same VAE noise in every run
        if tuple(t.shape) not in eps:
            eps[tuple(t.shape)] = torch.randn(t.shape, generator=gen)
        return eps[tuple(t.shape)].to(t.dtype)
    M.torch.randn_like = randn_like
    try:
        clean, nan, zero = three_runs(lambda: _emulated_run(kind, 6, 21))
    finally:
        M.torch.randn_like = orig
    for other in (nan, zero):
        assert other[0] == clean[0]
        assert other[1].keys() == clean[1].keys() and other[2].keys() == clean[2].keys() and len(clean[2]) > 100
        for k in clean[1]:
            assert torch.isfinite(clean[1][k]).all() and torch.equal(other[1][k], clean[1][k]), k
        for k in clean[2]:
            assert torch.isfinite(clean[2][k]).all() and torch.equal(other[2][k], clean[2][k]), k
    assert all(v == v and abs(v) < 1e6 for v in clean[0].values())
