"""Shared helpers for the parity tests."""
import glob
import os

import numpy as np
import torch

from deepsvg_amd import config as C
from deepsvg_amd.synthetic import det_state_dict

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    """the model / loss fixtures (tests/golden/make_golden.py); batch_assembly.npz belongs to the data path"""
    names = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
    return [n for n in names if not n.startswith("batch_") and n != "greedy_sample"]


BATCH_KEYS = ["commands", "args", "args_rel", "commands_grouped", "args_grouped", "args_rel_grouped", "filling"]


def golden_batch(tag):
    """tests/golden/batch_assembly.npz (make_golden_batch.py: outputs of the reference's SVGTensorDataset.get_data)
    -> (icons, fillings, (G, S, T), expected): icons[i] = list of group arrays [len, 14] float32 (the rows a
    .pkl file would hold, START_POS columns included); expected[key] = stacked reference outputs"""
    z = np.load(os.path.join(GOLDEN_DIR, "batch_assembly.npz"))
    G, S, T = (int(v) for v in z[f"{tag}/cfg"])
    rows, lens, n_groups, fills = (z[f"{tag}/{k}"] for k in ("rows", "lens", "n_groups", "fills"))
    icons, fillings, r, gi = [], [], 0, 0
    for n in n_groups:
        groups = []
        for j in range(n):
            groups.append(rows[r:r + lens[gi + j]].astype(np.float32))
            r += int(lens[gi + j])
        icons.append(groups)
        fillings.append([int(f) for f in fills[gi:gi + n]])
        gi += int(n)
    expected = {k: z[f"{tag}/{k}"].astype(np.int64 if k == "filling" else np.float32) for k in BATCH_KEYS}
    return icons, fillings, (G, S, T), expected


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False))


def build_cfg(kind):
    """same three configurations as tests/golden/make_golden.py (which builds them from the reference classes)"""
    if kind == "hier":
        cfg = C.Hierarchical()
        cfg.use_vae = False
    elif kind == "hier_vae":
        cfg = C.Hierarchical()
    elif kind == "onestage":
        cfg = C.OneStageOneShot()
        cfg.max_total_len = 50
        cfg.use_vae = False
    elif kind == "onestage240":
        cfg = C.OneStageOneShot()
        cfg.use_vae = False
    elif kind == "sketchformer240":
        cfg = C.Sketchformer()
        cfg.use_vae = False
    elif kind == "onestage_label":
        cfg = C.OneStageOneShot()
        cfg.max_total_len = 50
        cfg.label_condition = True
    elif kind == "hier_rel":
        cfg = C.Hierarchical()
        cfg.rel_targets = True
        cfg.use_vae = False
    elif kind == "sketchformer":    # deepsvg/model/config.py:74-80
        cfg = C.Sketchformer()
        cfg.max_total_len = 50
        cfg.use_vae = False
    elif kind == "selfmatch":       # deepsvg/model/config.py:101-108
        cfg = C.HierarchicalSelfMatching()
        cfg.use_vae = False
    elif kind == "fonts":           # ModelConfig of configs/deepsvg/hierarchical_ordered_fonts.py:4-9
        cfg = C.Hierarchical()
        cfg.label_condition = True
        cfg.dim_z = 128
    elif kind in WIDTH_KINDS:
        cfg = _width_cfg(kind)
    else:
        raise ValueError(kind)
    return cfg


# configurations off the default width (d_model 256 / 8 heads / dim_feedforward 512 / 8 groups of 30 commands): none of
# them fits a fused kernel, every layer takes the general kernels.  tests/golden/make_golden.py builds the same ones
# from the reference's classes for the two kinds that have a fixture (narrow128, narrow128_1s).
WIDTH_KINDS = ("narrow128", "narrow128_vae", "narrow128_1s", "narrow128_ar", "narrow128_match", "odd192", "odd192_1s",
               "odd96", "wide512", "ff1024", "nores")
ONE_STAGE_KINDS = ("onestage", "sketchformer", "onestage_label", "onestage240", "sketchformer240", "narrow128_1s",
                   "narrow128_ar", "odd192_1s")


def _set_width(cfg, d_model, n_heads, dim_ff, dim_z, layers, G=None, S=None, total=None):
    cfg.d_model, cfg.n_heads, cfg.dim_feedforward, cfg.dim_z = d_model, n_heads, dim_ff, dim_z
    cfg.n_layers = cfg.n_layers_decode = layers
    if G is not None:
        cfg.max_num_groups = cfg.num_groups_proposal = G
        cfg.max_seq_len = S
    cfg.max_total_len = total if total is not None else cfg.max_num_groups * cfg.max_seq_len
    cfg.use_vae = False
    return cfg


def _width_cfg(kind):
    if kind in ("narrow128", "narrow128_vae"):
        cfg = _set_width(C.Hierarchical(), 128, 4, 256, 128, 2, G=4, S=12)
        cfg.use_vae = kind == "narrow128_vae"
    elif kind == "narrow128_1s":        # 52 tokens on 4 heads
        cfg = _set_width(C.OneStageOneShot(), 128, 4, 256, 128, 2, total=50)
    elif kind == "narrow128_ar":        # causal, relative targets
        cfg = _set_width(C.Sketchformer(), 128, 4, 256, 128, 2, total=50)
    elif kind == "narrow128_match":     # (the oracle's loss needs num_groups_proposal == max_num_groups)
        cfg = _set_width(C.HierarchicalSelfMatching(), 128, 4, 256, 128, 2, G=4, S=12)
    elif kind == "odd192":              # 6 heads: no power of two, 32 % 6 != 0
        cfg = _set_width(C.Hierarchical(), 192, 6, 384, 256, 1, G=6, S=20)
    elif kind == "odd192_1s":           # 6 heads x 52 tokens: one head per workgroup
        cfg = _set_width(C.OneStageOneShot(), 192, 6, 384, 256, 1, total=50)
    elif kind == "odd96":               # 3 heads: one head per workgroup at every length
        cfg = _set_width(C.Hierarchical(), 96, 3, 192, 96, 1, G=4, S=12)
    elif kind == "wide512":
        cfg = _set_width(C.Hierarchical(), 512, 16, 1024, 64, 1)
    elif kind == "ff1024":              # fused attention fits, the fused FFN does not
        cfg = _set_width(C.Hierarchical(), 256, 8, 1024, 256, 1)
    elif kind == "nores":
        cfg = _set_width(C.Hierarchical(), 256, 8, 512, 256, 1)
        cfg.use_resnet = False
    else:
        raise ValueError(kind)
    return cfg


def width_batch(cfg, kind, n, seed):
    """-> (commands, args, args_dec) of n synthetic icons in the layout the kind's model takes"""
    from deepsvg_amd.synthetic import make_batch, make_batch_onestage
    if kind in ONE_STAGE_KINDS:
        commands, args = make_batch_onestage(n, total_len=cfg.max_total_len, seed=seed)
    else:
        commands, args = make_batch(n, G=cfg.max_num_groups, S=cfg.max_seq_len, seed=seed)
    args_dec = args
    if cfg.rel_targets:
        from oracle import batch_assembly_oracle as B
        args_dec = torch.stack([torch.stack([torch.from_numpy(B.relative_args(commands[i, g].numpy(), args[i, g].numpy()))
                                             for g in range(commands.shape[1])]) for i in range(n)])
    return commands, args, args_dec


def golden_args_dec(g, args):
    """decoder-side arguments: relative targets for rel_targets configs (model/config.py:52-53), else the same tensor"""
    return torch.from_numpy(g["args_dec"]) if "args_dec" in g else args


def check_sampled_sequences(cy, ay, g):
    """autoregressive samples against the reference's: the commands exactly; the arguments through their increments
    along the sequence - the draw at temperature 1e-4 is an arg-max except where two logits tie within ~1e-3, and one
    flipped relative argument shifts every later absolute coordinate (cumulative sum, model.py:461-479)"""
    want_c, want_a = torch.from_numpy(g["sample_commands"]), torch.from_numpy(g["sample_args"])
    assert torch.equal(cy.cpu(), want_c)
    got_d = torch.diff(ay.cpu().long(), dim=-2, prepend=torch.zeros_like(want_a[..., :1, :]))
    want_d = torch.diff(want_a.long(), dim=-2, prepend=torch.zeros_like(want_a[..., :1, :]))
    same = (got_d == want_d).float().mean().item()
    assert same > 0.99, f"only {same:.4f} of the sampled argument increments agree with the reference"


def golden_label(g):
    """class labels of a label-conditioned fixture (None otherwise)"""
    return torch.from_numpy(g["label"]) if "label" in g else None


def golden_setup(name):
    """-> (golden dict, cfg, commands, args, eps)"""
    g = load_golden(name)
    cfg = build_cfg(str(g["kind"]))
    commands = torch.from_numpy(g["commands"])
    args = torch.from_numpy(g["args"])
    eps = torch.from_numpy(g["eps"]) if "eps" in g else None
    return g, cfg, commands, args, eps


def weights_for(model, wseed):
    return det_state_dict(model, seed=int(wseed))


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def check_against_golden(g, out, losses=None, grads=None, *, logit_rtol=1e-3, logit_atol=1e-5, loss_tol=2e-5,
                         grad_norm_rtol=1e-3, grad_sample_atol=None, exact_argmax=True):
    """out: dict of CPU float tensors; grads: {name: tensor} or None"""
    cl = out["command_logits"].float()
    ref_cl = torch.from_numpy(g["command_logits"])
    assert torch.allclose(cl, ref_cl, rtol=logit_rtol, atol=logit_atol), \
        f"command_logits max err {(cl - ref_cl).abs().max().item():.3e}"
    if exact_argmax:
        assert torch.equal(cl.argmax(-1), ref_cl.argmax(-1)), "command argmax differs from the reference"
    al = out["args_logits"].float().reshape(-1)
    stride = int(g["args_logits_stride"])
    ref_s = torch.from_numpy(g["args_logits_sample"])
    assert torch.allclose(al[::stride], ref_s, rtol=logit_rtol, atol=logit_atol), \
        f"args_logits sample max err {(al[::stride] - ref_s).abs().max().item():.3e}"
    abssum = al.double().abs().sum().item()
    assert abs(abssum - float(g["args_logits_abssum"])) <= logit_rtol * float(g["args_logits_abssum"])
    if exact_argmax:
        am = out["args_logits"].float().argmax(-1).to(torch.int16)
        ref_am = torch.from_numpy(g["args_argmax"])
        agree = (am == ref_am).float().mean().item()
        assert agree > 0.9999, f"args argmax agreement {agree}"
    if "visibility_logits" in g:
        vl = out["visibility_logits"].float()
        ref_vl = torch.from_numpy(g["visibility_logits"])
        assert torch.allclose(vl, ref_vl, rtol=logit_rtol, atol=logit_atol)
    if losses is not None:
        for k in ("loss", "loss_cmd", "loss_args", "loss_visibility", "loss_kl"):
            if k in g:
                v = float(losses[k])
                assert abs(v - float(g[k])) <= loss_tol * max(1.0, abs(float(g[k]))), (k, v, float(g[k]))
    if grads is not None:
        names = [str(n) for n in g["grad_names"]]
        norms = g["grad_norms"]
        samples = g["grad_samples"]
        for i, n in enumerate(names):
            gr = grads[n].double().reshape(-1)
            ref_norm = float(norms[i])
            assert abs(gr.norm().item() - ref_norm) <= grad_norm_rtol * max(ref_norm, 1e-8), \
                (n, gr.norm().item(), ref_norm)
            idx = torch.linspace(0, gr.numel() - 1, 16).long()
            s = gr[idx].float()
            ref_sample = torch.from_numpy(samples[i])
            rms = ref_norm / max(gr.numel(), 1) ** 0.5
            atol = grad_sample_atol if grad_sample_atol is not None else 5e-3 * rms + 1e-6
            assert torch.allclose(s, ref_sample, rtol=2e-3, atol=atol), (n, (s - ref_sample).abs().max().item())


# ---- one-shot greedy_sample fixtures (tests/golden/make_golden_sample.py) ------------------------------------------
SAMPLE_TIE = 2e-3       # the reference draws from Categorical(logits / 1e-4): slots whose two best logits lie closer are near-ties


def sample_cases():
    return ["hier5", "fonts4"]


def sample_fixture(tag):
    """-> (dict of that case's arrays as tensors, cfg)"""
    z = np.load(os.path.join(GOLDEN_DIR, "greedy_sample.npz"), allow_pickle=False)
    g = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(tag + "/")}
    cfg = build_cfg(str(g["kind"]))
    t = {k: (torch.from_numpy(v.astype(np.int64)) if v.dtype == np.int16 else
             torch.from_numpy(v.astype(np.float32)) if v.dtype == np.float16 else
             torch.from_numpy(v) if v.dtype.kind in "fi" and v.ndim else v) for k, v in g.items()}
    return t, cfg


def check_sample(got_c, got_a, want_c, want_a, cmd_gap, args_gap):
    """commands / arguments equal to the reference's draw wherever that draw is not a near-tie (a flipped command also
    changes which argument slots are valid, so arguments are compared under safe commands)"""
    got_c, got_a = got_c.cpu().long(), got_a.cpu().long()
    assert got_c.shape == want_c.shape and got_a.shape == want_a.shape
    okc = cmd_gap > SAMPLE_TIE
    assert torch.equal(got_c[okc], want_c[okc]), "sampled commands differ from the reference outside near-ties"
    oka = (args_gap > SAMPLE_TIE) & okc.unsqueeze(-1)
    assert torch.equal(got_a[oka], want_a[oka]), "sampled arguments differ from the reference outside near-ties"
    assert okc.float().mean().item() > 0.98 and oka.float().mean().item() > 0.95     # the check is not vacuous


def run_sample_checks(sample_fn, t, cfg, device="cpu", eps_ctx=None):
    """sample_fn(commands, args, label, z, hierarch_logits, concat_groups, icon) -> (commands_y, args_y); every leg of
    the fixture: from the inputs, from z, forced visibility (one visible group / none), concat_groups per icon"""
    dev = lambda x: x.to(device) if torch.is_tensor(x) else x                       # noqa: E731
    label = dev(t["label"]) if "label" in t else None
    c, a = dev(t["commands"]), dev(t["args"])
    cy, ay = sample_fn(c, a, label, None, None, False, None)
    check_sample(cy, ay, t["cy"], t["ay"], t["cmd_gap"], t["args_gap"])
    cy, ay = sample_fn(None, None, label, dev(t["z"]), None, False, None)
    check_sample(cy, ay, t["cy_z"], t["ay_z"], t["cmd_gap"], t["args_gap"])
    cy, ay = sample_fn(None, None, label, dev(t["hz"]), dev(t["hl"]), False, None)
    check_sample(cy, ay, t["cy_h"], t["ay_h"], t["cmd_gap_h"], t["args_gap_h"])
    inv = torch.tensor([0] + [4] * 30)
    assert torch.equal(cy[1].cpu().long(), inv.expand(8, 31)) and bool((ay[1] == -1).all())
    assert all(torch.equal(cy[0, g].cpu().long(), inv) for g in range(8) if g != 3)
    off = 0
    for i, n_tok in enumerate(t["cat_len"].tolist()):
        li = label[i:i + 1] if label is not None else None
        c1, a1 = sample_fn(c[i:i + 1], a[i:i + 1], li, None, None, True, i)
        assert c1.shape == (1, n_tok) and a1.shape == (1, n_tok, cfg.n_args)
        if bool((t["cmd_gap"][i] > SAMPLE_TIE).all()) and bool((t["args_gap"][i] > SAMPLE_TIE).all()):
            assert torch.equal(c1[0].cpu().long(), t["cat_c"][off:off + n_tok])
            assert torch.equal(a1[0].cpu().long(), t["cat_a"][off:off + n_tok])
        off += n_tok
