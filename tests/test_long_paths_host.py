"""Two-stage configs with paths of up to 254 commands (max_seq_len + 2 <= 256), host side, on CPU: construction and
parameter layout, the limits that remain, and - with the ops replaced by plain-torch restatements (tests/torch_ops_ref.py
+ tests/long_ops_ref.py) - the host logic of the path-level stages against the reference golden
tests/golden/long/hier_long100_n3.npz."""
import os

import numpy as np
import pytest
import torch

import deepsvg_amd
from oracle import svg_transformer_oracle as O
from tests import helpers as H
from tests import long_ops_ref as LR

GOLDEN = os.path.join(H.GOLDEN_DIR, "long", "hier_long100_n3.npz")


def _shapes(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("max_seq_len", [63, 100, 254])
def test_hierarchical_with_long_paths_constructs(max_seq_len):
    model = deepsvg_amd.SVGTransformer(LR.long_cfg(max_seq_len))
    got, base = _shapes(model), _shapes(deepsvg_amd.SVGTransformer(LR.long_cfg(30)))
    assert list(got) == list(base)
    # only the path-level positional tables grow, by the change of max_seq_len
    for k in got:
        if got[k] != base[k]:
            assert ("pos_encoding" in k or ".PE." in k) and got[k][1:] == base[k][1:] and got[k][0] - base[k][0] == max_seq_len - 30, k
    # the reference's own parameter names and order (grad_names of the golden, recorded from the reference at 100)
    names = [n for n, _ in model.named_parameters()]
    assert names == [str(n) for n in np.load(GOLDEN)["grad_names"]]


def test_paths_of_255_commands_are_refused():
    with pytest.raises(NotImplementedError):
        deepsvg_amd.SVGTransformer(LR.long_cfg(255))


def test_self_matching_with_long_paths_is_refused():
    with pytest.raises(NotImplementedError, match="Hungarian"):
        deepsvg_amd.SVGTransformer(LR.long_cfg(100, "selfmatch"))
    deepsvg_amd.SVGTransformer(LR.long_cfg(62, "selfmatch"))


@pytest.fixture
def long_ops(emulated_ops):
    saved = LR.install()
    yield
    LR.restore(saved)


def _golden():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    return g, LR.long_cfg(100), torch.from_numpy(g["commands"]), torch.from_numpy(g["args"])


def _run(cfg, sd, commands, args, pack):
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(sd)
    model.pack_encoder = pack
    model.eval()
    loss_fn = deepsvg_amd.SVGLoss(cfg)
    out = model(commands, args, commands, args, params={})
    ld = loss_fn(out, None, weights=O.DEFAULT_WEIGHTS)
    ld["loss"].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return model, {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}, ld, grads


@pytest.mark.parametrize("pack", [True, False])
def test_long_paths_match_golden_with_emulated_ops(pack, long_ops):
    g, cfg, commands, args = _golden()
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), g["wseed"])
    model, out, ld, grads = _run(cfg, sd, commands, args, pack)
    assert (model.last_packing is not None) == pack
    H.check_against_golden(g, out, {k: v.item() for k, v in ld.items()}, grads, logit_rtol=1e-4, logit_atol=1e-5,
                           loss_tol=1e-5, grad_norm_rtol=2e-4)
    with torch.no_grad():
        z = model(commands, args, commands, args, encode_mode=True)
        hl, zg = model(commands, args, commands, args, return_hierarch=True)
    assert torch.allclose(z, torch.from_numpy(g["z"]), rtol=1e-4, atol=1e-5)
    assert torch.allclose(hl, torch.from_numpy(g["hier_logits"]), rtol=1e-4, atol=1e-5)
    assert torch.allclose(zg, torch.from_numpy(g["hier_z"]), rtol=1e-4, atol=1e-5)


def test_packed_and_padded_encoders_agree(long_ops):
    from deepsvg_amd.synthetic import make_batch
    cfg = LR.long_cfg(126)
    commands, args = make_batch(3, 8, 126, seed=7)
    sd = H.weights_for(deepsvg_amd.SVGTransformer(cfg), 99)
    outs = []
    for pack in (True, False):
        model = deepsvg_amd.SVGTransformer(cfg)
        model.load_state_dict(sd)
        model.pack_encoder = pack
        model.eval()
        with torch.no_grad():
            outs.append(model(commands, args, commands, args, encode_mode=True))
    assert torch.allclose(outs[0], outs[1], rtol=1e-4, atol=2e-5)


def test_long_path_masks_and_packing_restatements():
    """the restated masks equal the existing ones where both apply (paths of <= 62 commands)"""
    from tests import torch_ops_ref as ref
    from deepsvg_amd.synthetic import make_batch
    commands, args = make_batch(4, 8, 62, seed=3)
    cmd = commands.view(-1, 64)
    km, vis, gm = ref.build_masks(cmd, 64, 8, 4, want_group_mask=True)
    lens, vis2, gm2 = LR.build_masks_lens(cmd, 64, 8, 4, want_group_mask=True)
    assert torch.equal(lens, ref.seq_lens(cmd, 64)) and torch.equal(vis, vis2) and torch.equal(gm, gm2)
    a = args.reshape(-1, args.shape[-1])
    for x, y in zip(ref.pack_tokens(cmd.reshape(-1), a, km, 32, 64), LR.pack_tokens_lens(cmd.reshape(-1), a, lens, 32, 64)):
        assert torch.equal(x, y)
