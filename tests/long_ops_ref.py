"""Plain-torch restatements of the ops added for two-stage configs with paths of 65..256 tokens (ops.build_masks_lens,
ops.pack_tokens_lens, and the S > 64 packed / path-stage routes of attention_fwd / bwd and masked_mean_fwd / bwd), to be
installed on top of the emulated_ops fixture (tests/torch_ops_ref.py restates the ops that existed before them)."""
import torch

from tests import torch_ops_ref as ref

LONG_CONFIG_SEED = 1234


def long_cfg(max_seq_len, kind="hier"):
    from deepsvg_amd import config as C
    if kind == "hier":
        cfg = C.Hierarchical()
        cfg.use_vae = False
    elif kind == "fonts":       # configs/deepsvg/hierarchical_ordered_fonts.py:4-9
        cfg = C.Hierarchical()
        cfg.label_condition = True
        cfg.dim_z = 128
        cfg.use_vae = False         # (deterministic: no reparametrisation draw)
    elif kind == "selfmatch":
        cfg = C.HierarchicalSelfMatching()
        cfg.use_vae = False
    else:
        raise ValueError(kind)
    cfg.max_seq_len = max_seq_len
    return cfg


def build_masks_lens(commands, S, G=0, eos_id=4, want_group_mask=False):
    cmd = commands.view(-1, S)
    is_eos = cmd.long() == eos_id
    lens = ((is_eos.cumsum(1) == 0).sum(1)).to(torch.int32)
    seq_visible = (is_eos.sum(1) < S - 1).to(torch.int32)
    group_mask = None
    if want_group_mask:
        wg = 1 << torch.arange(G, dtype=torch.int64, device=cmd.device)
        group_mask = (seq_visible.view(-1, G).long() * wg).sum(1)
    return lens, seq_visible, group_mask


def pack_tokens_lens(commands, args, lens, n_seq, S):
    valid = torch.arange(S, device=commands.device).unsqueeze(0) < lens.long().unsqueeze(1)
    seq_off = torch.zeros(n_seq + 1, dtype=torch.int32, device=commands.device)
    seq_off[1:] = torch.cumsum(lens.long(), 0).to(torch.int32)
    total = int(seq_off[-1])
    cap = n_seq * S
    a = args.reshape(cap, -1)
    sel = valid.reshape(-1).nonzero().squeeze(1)
    pcmd = commands.reshape(-1)[0].repeat(cap).clone()
    parg = a[0:1].repeat(cap, 1).clone()
    ppos = torch.zeros(cap, dtype=torch.int32, device=commands.device)
    pcmd[:total] = commands.reshape(-1)[sel]
    parg[:total] = a[sel]
    ppos[:total] = (sel % S).to(torch.int32)
    return seq_off, pcmd, parg, ppos


def attention_fwd(qkv, key_mask, n_seq, S, n_heads, scale, drop_p=0.0, drop_site=0, seed=None, seq_off=None, tiles=None,
                  causal=False, only_row=None, out=None, path_stage=False):
    if seq_off is not None and S > 64:      # (the restatement's packed route holds lengths in 64-bit masks)
        dense, idx, lens = ref._unpack_rows(qkv, seq_off, n_seq, S)
        o = ref.attention_fwd(dense, lens.to(torch.int32), n_seq, S, n_heads, scale, drop_p, drop_site, seed)
        return ref._repack_rows(o, idx, qkv.shape[0])
    return ref.attention_fwd(qkv, key_mask, n_seq, S, n_heads, scale, drop_p, drop_site, seed, seq_off, tiles, causal,
                             only_row, out)


def attention_bwd(qkv, key_mask, dout, n_seq, S, n_heads, scale, drop_p=0.0, drop_site=0, seed=None, seq_off=None,
                  tiles=None, causal=False, path_stage=False):
    if seq_off is not None and S > 64:
        dense, idx, lens = ref._unpack_rows(qkv, seq_off, n_seq, S)
        ddense, _, _ = ref._unpack_rows(dout, seq_off, n_seq, S)
        g = ref.attention_bwd(dense, lens.to(torch.int32), ddense, n_seq, S, n_heads, scale, drop_p, drop_site, seed)
        return ref._repack_rows(g, idx, qkv.shape[0])
    return ref.attention_bwd(qkv, key_mask, dout, n_seq, S, n_heads, scale, drop_p, drop_site, seed, seq_off, tiles, causal)


def masked_mean_fwd(x, mask, n_seq, S, seq_off=None):
    if seq_off is not None and S > 64:
        dense, _, lens = ref._unpack_rows(x, seq_off, n_seq, S)
        return ref.masked_mean_fwd(dense, lens.to(torch.int32), n_seq, S)
    return ref.masked_mean_fwd(x, mask, n_seq, S, seq_off)


def masked_mean_bwd(dout, mask, n_seq, S, seq_off=None, total_rows=None):
    if seq_off is not None and S > 64:
        probe = torch.zeros((int(total_rows), 1), dtype=dout.dtype, device=dout.device)
        _, idx, lens = ref._unpack_rows(probe, seq_off, n_seq, S)
        return ref._repack_rows(ref.masked_mean_bwd(dout, lens.to(torch.int32), n_seq, S), idx, int(total_rows))
    return ref.masked_mean_bwd(dout, mask, n_seq, S, seq_off, total_rows)


NAMES = ("build_masks_lens", "pack_tokens_lens", "attention_fwd", "attention_bwd", "masked_mean_fwd", "masked_mean_bwd")


def install():
    """on top of tests/conftest.py's emulated_ops: -> the replaced functions, for restore()"""
    import deepsvg_amd.ops as ops
    saved = {n: getattr(ops, n) for n in NAMES}
    g = globals()
    for n in NAMES:
        setattr(ops, n, g[n])
    return saved


def restore(saved):
    import deepsvg_amd.ops as ops
    for n, fn in saved.items():
        setattr(ops, n, fn)
