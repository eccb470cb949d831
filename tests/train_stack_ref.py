"""Train-mode gradients of one transformer stack (SVGTransformer._run_stack, dropout on) against torch autograd.

`stack_reference` is a straight-line float64 forward of the pre-LN stack whose dropout masks are multiplier tensors built from
the draw restatements of tests/torch_ops_ref.py (`R.drop_mult`, `R.drop2_mult`, `R._attn_drop` and the id helpers - the
functions the kernel tests pin to the kernels bit for bit).  Its backward is autograd's: it calls none of the restated
backward ops, so a wrong site id, a stale masked hand-off or a mask indexed from the wrong row base in
deepsvg_amd/functional.py shows up as a difference, not as a plausible gradient.

CASES is the table of stack calls both test files run (tests/test_train_stack_host.py with the restatements installed in
place of `ops`, tests/test_train_stack_gpu.py on the kernels); FRONT_CASES the short table of the dropout front ends
(EmbedFn, PackedEmbedFn, AddPosFn) with `front_reference`.  `run_stack_case` / `run_front_case` push a case through the
product with whatever `ops` holds at the time and count the launches the case names."""
import contextlib
import dataclasses
import os

import torch

from tests import torch_ops_ref as R

SEED = 0x0123456789ABCDEF       # both 32-bit halves non-zero: the hi half enters the draws' second mixing constant
DROP_P = 0.1
WRONG = 1000                    # `wrong_site=s`: that site alone draws from s + WRONG ("all": every site does)
FP32_BOUND = 1e-3               # the project's parity tolerance of the fp32 path (tests/test_model_gpu.py)
BF16_FACTOR = 3.0               # bf16: bound(tensor) = BF16_FACTOR x d_round(tensor), d_round from the emulated bf16 run


@dataclasses.dataclass
class Case:
    name: str
    dtype: str                      # "fp32" | "bf16"
    kind: str                       # tests/helpers.build_cfg kind, or "long126"
    stack: str                      # attribute path of the stack inside the model
    n_layers: int
    n_seq: int
    S: int
    site: int = 100
    key_bits: list = None           # per sequence: bit j set = key j visible (int64 key bitmask), or
    key_lens: list = None           # valid-prefix lengths (int32, the S > 64 layout), or
    packed_lens: list = None        # packed layout: sequence lengths (seq_off / tiles); rows rounded up to 128
    causal: bool = False
    z: bool = False
    l: bool = False
    live: tuple = None              # (n_live sequences, R rows): backward over the row prefix; dout zero past n_live * S
    hoist: bool = True
    min_rows: int = None            # Fn.FFN_MIN_ROWS = Fn.ATTN_MIN_ROWS (None: the defaults, i.e. nothing fused here)
    gs_stack: bool = True           # Fn.GS_STACK
    ln_masked: bool = True          # Fn.LN_BWD_MASKED
    path_stage: bool = False
    ffn_ids: object = "plain"       # hidden-site draw ids: "plain" | "fused" | R0 (rows below R0 fused, the rest plain)
    expect: dict = dataclasses.field(default_factory=dict)      # counter -> ">0" | 0 (see _Counters); "gpu:" prefix: device only

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"

    @property
    def rows(self):
        if self.packed_lens is not None:
            return min((sum(self.packed_lens) + 127) // 128 * 128, self.n_seq * self.S)
        return self.n_seq * self.S

    def sites(self):
        """every dropout site the case draws from"""
        out = []
        for i in range(self.n_layers):
            s0 = self.site + 8 * i
            out += [s0, s0 + 1, s0 + 3, s0 + 4] + ([s0 + 2] if self.z else []) + ([s0 + 5] if self.l else [])
        return sorted(out)


def _lens_bits(lens):
    return [(1 << n) - 1 for n in lens]


_LENS6 = [1, 30, 17, 8, 30, 23]                                     # 6 x 30 with key mask: lengths include 1 and 30
_LENS16 = [1, 30, 17, 8, 30, 23, 2, 29, 12, 30, 5, 19, 30, 26, 9, 14]
_GROUP_BITS16 = [0x01, 0xFF, 0x3D, 0x80, 0x5A, 0x07, 0xF0, 0x81, 0x13, 0xFE, 0x20, 0xAB, 0x7F, 0x44, 0xC3, 0x19]
_UNFUSED = {"attn_block_fwd": 0, "ffn_fwd": 0, "gs_layer_fwd": 0, "gs_stack_fwd": 0}


def _cases():
    c = []
    for dt in ("fp32", "bf16"):
        # (the conditioning add's backward replays the attention residual's mask itself, `mask_site=`, on bf16 rows only)
        ms = ({"bcast_add_bwd_mask_site": ">0", "drop_apply_attn_res": 0} if dt == "bf16" else
              {"bcast_add_bwd_mask_site": 0, "drop_apply_attn_res": ">0"})
        c.append(Case("unfused_masked", dt, "hier", "encoder.encoder", 2, 6, 30, key_bits=_lens_bits(_LENS6),
                      expect={**_UNFUSED, "ln_bwd_masked": ">0", "drop_apply_ffn_res": 0}))
        c.append(Case("unfused_no_handoff", dt, "hier", "encoder.encoder", 2, 6, 30, key_bits=_lens_bits(_LENS6), ln_masked=False,
                      expect={**_UNFUSED, "ln_bwd_masked": 0, "drop_apply_ffn_res": ">0"}))
        c.append(Case("label", dt, "fonts", "decoder.decoder", 2, 6, 30, site=400, z=True, l=True,
                      expect={**_UNFUSED, "bcast_add_bwd_label": ">0", **ms}))
        for hoist in (True, False):
            c.append(Case("decoder_z" + ("" if hoist else "_wg"), dt, "hier", "decoder.decoder", 2, 6, 30, site=400, z=True,
                          hoist=hoist, expect={**_UNFUSED, **ms}))
        c.append(Case("decoder_live", dt, "hier", "decoder.decoder", 2, 6, 30, site=400, z=True, live=(3, 128),
                      expect={**_UNFUSED, **ms, "ln_bwd_prefix_only": ">0", "ln_bwd_full": 0}))
        c.append(Case("causal", dt, "sketchformer", "decoder.decoder", 2, 6, 30, site=400, key_bits=_lens_bits(_LENS6), z=True,
                      causal=True, expect={**_UNFUSED, "attention_fwd_causal": ">0", "attention_bwd_causal": ">0"}))
    fused = {"attn_block_fwd": ">0", "ffn_fwd_train": ">0", "gs_layer_fwd": 0, "gs_stack_fwd": 0, "ffn_bwd_dx": ">0",
             "gpu:ffn_gate_dw2": ">0", "ln_bwd_masked": ">0"}
    c.append(Case("fused_dense", "bf16", "hier", "encoder.encoder", 2, 16, 30, key_bits=_lens_bits(_LENS16), min_rows=256,
                  ffn_ids="fused", expect={**fused, "attention_bwd_outproj": ">0", "attention_bwd": 0}))
    c.append(Case("fused_short", "bf16", "hier", "encoder.encoder", 2, 64, 8, min_rows=256, ffn_ids="fused",
                  key_bits=[((0x9D * (i + 3)) & 0xFF) | 1 for i in range(64)],
                  expect={**fused, "attention_bwd_outproj": 0, "attention_bwd": ">0"}))
    c.append(Case("fused_z", "bf16", "hier", "decoder.decoder", 2, 16, 30, site=400, z=True, min_rows=256, ffn_ids="fused",
                  expect={**fused, "attn_block_fwd_seq_add": ">0", "bcast_add_fwd_": 0, "attention_bwd_outproj": ">0"}))
    c.append(Case("fused_z_live", "bf16", "hier", "decoder.decoder", 2, 16, 30, site=400, z=True, min_rows=256, ffn_ids="fused",
                  live=(4, 128), expect={**{k: v for k, v in fused.items() if k != "gpu:ffn_gate_dw2"},
                                         "attn_block_fwd_seq_add": ">0", "attention_bwd_outproj": 0, "attention_bwd": ">0",
                                         "ln_bwd_full": 0}))
    c.append(Case("fused_packed", "bf16", "hier", "encoder.encoder", 2, 30, 30, packed_lens=list(range(1, 31)), min_rows=256,
                  ffn_ids="fused", expect={**fused, "attn_block_fwd_packed": ">0", "attention_bwd_outproj": ">0",
                                           "attention_bwd": 0}))
    for stack_on in (True, False):
        exp = ({"gs_stack_fwd": ">0", "gs_stack_bwd": ">0"} if stack_on else
               {"gs_stack_fwd": 0, "gs_layer_fwd": ">0", "gs_layer_bwd": ">0"})
        exp = {**exp, "attn_block_fwd": 0, "ffn_fwd": 0, "ln_bwd_masked": 0}
        tag = "gs_stack" if stack_on else "gs_layer"
        c.append(Case(tag + "_enc", "bf16", "hier", "encoder.hierarchical_encoder", 2, 16, 8, site=200, key_bits=_GROUP_BITS16,
                      gs_stack=stack_on, expect=exp))
        c.append(Case(tag + "_dec", "bf16", "hier", "decoder.hierarchical_decoder", 2, 16, 8, site=300, z=True,
                      gs_stack=stack_on, expect=exp))
    c.append(Case("split_remainder", "bf16", "hier", "decoder.decoder", 1, 2048 + 5, 8, site=400, z=True, min_rows=1024,
                  ffn_ids=2048 * 8, expect={"attn_block_fwd": ">0", "ffn_fwd_train": ">0", "gs_layer_fwd_tail": ">0",
                                            "ffn_bwd_dx": ">0", "attention_bwd": ">0", "gpu:ffn_gate_dw2": ">0"}))
    c.append(Case("long_path", "bf16", "long126", "encoder.encoder", 2, 3, 128, key_lens=[1, 77, 128], path_stage=True,
                  expect={**_UNFUSED, "attention_fwd_path_stage": ">0", "attention_bwd_path_stage": ">0",
                          "gpu:long_route_mfma": ">0"}))
    return c


CASES = _cases()


# ----------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------
def make_inputs(case, dim_z=256, dim_label=64):
    """-> dict of CPU fp32 tensors x, dout [, z, l]; a bf16 case rounds them to bf16 (the reference reads the rounded values)"""
    g = torch.Generator().manual_seed(20240611)
    rows = case.rows
    t = {"x": torch.randn(rows, 256, generator=g), "dout": torch.randn(rows, 256, generator=g)}
    if case.z:
        t["z"] = 0.5 * torch.randn(case.n_seq, dim_z, generator=g)
    if case.l:
        t["l"] = torch.randn(case.n_seq, dim_label, generator=g)
    if case.live is not None:
        t["dout"][case.live[0] * case.S:] = 0          # a loss that ignores the sequences past the live prefix
    if case.packed_lens is not None:
        t["dout"][sum(case.packed_lens):] = 0           # nothing reads the inert rows (the masked mean-pool skips them)
    if case.dtype == "bf16":
        t = {k: v.to(torch.bfloat16).float() for k, v in t.items()}
    return t


def _valid_keys(case):
    """bool [n_seq, S] of the visible keys, or None"""
    j = torch.arange(case.S)
    if case.key_bits is not None:
        return ((torch.tensor(case.key_bits, dtype=torch.int64).unsqueeze(1) >> j) & 1).bool()
    lens = case.key_lens if case.key_lens is not None else case.packed_lens
    if lens is not None:
        return j.unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
    return None


def _packed_index(case):
    """dense row n * S + pos of every packed row"""
    return torch.cat([n * case.S + torch.arange(ln) for n, ln in enumerate(case.packed_lens)])


# ----------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------
def _ln(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + eps) * g + b


_MASKS = {}          # (case id, kind, site) -> multiplier tensor: the wrong-site passes of a case redraw one site only


def _mask(case, kind, seed, site):
    """multiplier tensor of one dropout site, from the draw restatements alone"""
    if _MASKS and next(iter(_MASKS))[0] != case.id:
        _MASKS.clear()
    key = (case.id, kind, site)
    if key not in _MASKS:
        dev, rows = torch.device("cpu"), case.rows
        if kind == "row":           # the two residual sites: element (row, column) of the [rows, 256] activation
            m = R.drop_mult(DROP_P, seed, site, R._ids(rows, 256, dev))
        elif kind == "seq":         # the conditioning rows: element (sequence, column), before the broadcast
            m = R.drop_mult(DROP_P, seed, site, R._ids(case.n_seq, 256, dev))
        elif kind == "hidden":      # the unfused and group-stage launches: element (row, unit) of the [rows, 512] hidden layer
            m = R.drop_mult(DROP_P, seed, site, R._ids(rows, 512, dev))
        elif kind == "hidden_fused":    # the fused FFN kernels: draw scheme v2 over the ids in the order their lanes own them
            m = R.drop2_mult(DROP_P, seed, site, R._ffn_hidden_ids(rows, dev))
        else:                       # attention probabilities, dense (sequence, head, query, key) coordinates
            m = R._attn_drop(DROP_P, seed, site, case.n_seq, case.S, 8, dev)
        _MASKS[key] = m
    return _MASKS[key].double()


def stack_reference(case, params, x, z, l, dout, seed, wrong_site=None):
    """float64 autograd over the straight-line stack.  params: {name inside the stack: tensor} (what the product multiplies
    with: the bf16 images of a bf16 case); seed: int64[1] CPU tensor.  -> {"out", "dx" [, "dz", "dl"], "grad:<name>"}"""
    S, n_seq, H = case.S, case.n_seq, 8
    assert int(seed.reshape(-1)[0]) == SEED
    wrong = set(case.sites()) if wrong_site == "all" else {wrong_site}             # ("all": every site redrawn at once)
    site_of = lambda s: s + WRONG if s in wrong else s                             # noqa: E731
    f64 = lambda t: None if t is None else t.detach().double().cpu().clone().requires_grad_()      # noqa: E731
    x, z, l = f64(x), f64(z), f64(l)
    P = {k: f64(v) for k, v in params.items()}
    rows = x.shape[0]
    assert rows == case.rows
    valid = _valid_keys(case)
    scale = float(256 // H) ** -0.5
    pidx = _packed_index(case) if case.packed_lens is not None else None

    def attention(qkv, s0):
        if pidx is not None:        # packed rows unpack into zero-padded dense sequences; rows past the last token give zeros
            qkv = torch.zeros((n_seq * S, 768), dtype=qkv.dtype).index_copy(0, pidx, qkv[:pidx.numel()])
        q, k, v = qkv.view(n_seq, S, 3, H, 32).permute(2, 0, 3, 1, 4)
        s = (q * scale) @ k.transpose(-1, -2)
        if case.causal:
            s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1), float("-inf"))
        if valid is not None:
            s = s.masked_fill(~valid.view(n_seq, 1, 1, S), float("-inf"))
        pr = torch.softmax(s, -1) * _mask(case, "attn", seed, site_of(s0))
        o = (pr @ v).permute(0, 2, 1, 3).reshape(n_seq * S, 256)
        if pidx is not None:
            o = torch.cat([o[pidx], torch.zeros((rows - pidx.numel(), 256), dtype=o.dtype)])
        return o

    cur = x
    for i in range(case.n_layers):
        s0, w = case.site + 8 * i, f"layers.{i}."
        m_res1 = _mask(case, "row", seed, site_of(s0 + 1))
        m_res2 = _mask(case, "row", seed, site_of(s0 + 4))
        if case.ffn_ids == "plain":
            m_hid = _mask(case, "hidden", seed, site_of(s0 + 3))
        else:
            m_hid = _mask(case, "hidden_fused", seed, site_of(s0 + 3))
            if case.ffn_ids != "fused":     # remainder split: the tail rows draw from the plain ids, counted from the buffer's first row
                m_hid = torch.where((torch.arange(rows) < int(case.ffn_ids)).unsqueeze(1), m_hid,
                                    _mask(case, "hidden", seed, site_of(s0 + 3)))
        xn1 = _ln(cur, P[w + "norm1.weight"], P[w + "norm1.bias"])
        qkv = xn1 @ P[w + "self_attn.in_proj_weight"].t() + P[w + "self_attn.in_proj_bias"]
        ao = attention(qkv, s0)
        x1 = cur + m_res1 * (ao @ P[w + "self_attn.out_proj.weight"].t() + P[w + "self_attn.out_proj.bias"])
        if z is not None:
            g = (z @ P[w + "linear_global.weight"].t() + P[w + "linear_global.bias"]) * _mask(case, "seq", seed, site_of(s0 + 2))
            x1 = x1 + g.repeat_interleave(S, 0)
        if l is not None:
            g2 = (l @ P[w + "linear_global2.weight"].t() + P[w + "linear_global2.bias"]) * _mask(case, "seq", seed, site_of(s0 + 5))
            x1 = x1 + g2.repeat_interleave(S, 0)
        xn2 = _ln(x1, P[w + "norm2.weight"], P[w + "norm2.bias"])
        h = m_hid * torch.relu(xn2 @ P[w + "linear1.weight"].t() + P[w + "linear1.bias"])
        cur = x1 + m_res2 * (h @ P[w + "linear2.weight"].t() + P[w + "linear2.bias"])
    out = _ln(cur, P["norm.weight"], P["norm.bias"])
    out.backward(dout.detach().double().cpu())
    res = {"out": out.detach(), "dx": x.grad}
    if z is not None:
        res["dz"] = z.grad
    if l is not None:
        res["dl"] = l.grad
    for k, v in P.items():
        if v.grad is not None:
            res["grad:" + k] = v.grad
    return res


# ----------------------------------------------------------------------------------------------------
# what is compared
# ----------------------------------------------------------------------------------------------------
def compared(case, res):
    """the tensors of a result (reference or product) the case compares: valid rows of a packed layout, prefix rows of dx under
    a live prefix, everything else whole"""
    out = {k: v.detach().double().cpu() for k, v in res.items()}
    if case.packed_lens is not None:
        n = sum(case.packed_lens)
        out["out"], out["dx"] = out["out"][:n], out["dx"][:n]
    if case.live is not None and "dx" in out:
        out["dx"] = out["dx"][:case.live[1]]
    return out


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def distances(case, got, ref):
    """{tensor name: relative L2 distance to the reference} over the compared tensors (every tensor of the reference must be there)"""
    g, r = compared(case, got), compared(case, ref)
    missing = sorted(set(r) - set(g))
    assert not missing, f"{case.id}: the product returned no {missing}"
    return {k: rel_l2(g[k], r[k]) for k in r}


def exact_zeros(case, res):
    """the exact zeros the table names: -> list of (what, tensor that must be all zero)"""
    z = []
    if isinstance(case, FrontCase):
        pos = res["grad:pos"]
        return [("position-table gradient rows past S", pos[case.S:])] if pos.shape[0] > case.S else []
    if case.packed_lens is not None:
        z.append(("dx of the inert packed rows", res["dx"][sum(case.packed_lens):]))
    if case.live is not None:
        z.append(("dz of the sequences past the live prefix", res["dz"][case.live[0]:]))
        z.append(("dx rows of the prefix past the last live sequence", res["dx"][case.live[0] * case.S:case.live[1]]))
    return z


# ----------------------------------------------------------------------------------------------------
# a case through the product
# ----------------------------------------------------------------------------------------------------
class _Counters:
    """wraps functions of deepsvg_amd.ops (whatever is installed: kernels or restatements) and counts the launches the cases name"""

    NAMES = ("attn_block_fwd", "ffn_fwd", "ffn_bwd_dx", "ffn_gate_dw2", "attention_fwd", "attention_bwd", "attention_bwd_outproj",
             "gs_layer_fwd", "gs_layer_bwd", "gs_stack_fwd", "gs_stack_bwd", "drop_apply", "bcast_add_fwd_", "bcast_add_bwd",
             "layernorm_bwd", "_long_route", "add_pos_fwd", "add_pos_bwd", "embed_gather", "embed_scatter")

    def __init__(self, case):
        self.case, self.n, self.saved = case, {}, {}

    def hit(self, key):
        self.n[key] = self.n.get(key, 0) + 1

    def _note(self, name, a, kw, ret):
        c = self.case
        self.hit(name)
        if name == "attn_block_fwd":
            if kw.get("seq_add") is not None:
                self.hit("attn_block_fwd_seq_add")
            if kw.get("seq_off") is not None and kw.get("tiles") is not None:
                self.hit("attn_block_fwd_packed")
        elif name == "ffn_fwd" and kw.get("train"):
            self.hit("ffn_fwd_train")
        elif name == "gs_layer_fwd" and kw.get("seq_base") and kw.get("ffn_format"):
            self.hit("gs_layer_fwd_tail")
        elif name in ("attention_fwd", "attention_bwd"):
            if kw.get("causal"):
                self.hit(name + "_causal")
            if kw.get("path_stage"):
                self.hit(name + "_path_stage")
        elif name == "_long_route" and ret == "mfma":
            self.hit("long_route_mfma")
        elif name == "drop_apply":          # (x, p, site, seed)
            k = (int(a[2]) - c.site) % 8
            if k == 4:
                self.hit("drop_apply_ffn_res")
            if k == 1:
                self.hit("drop_apply_attn_res")
        elif name == "bcast_add_bwd":       # (dx, n_seq, S, p, site, seed, ...)
            if kw.get("mask_site") is not None:
                self.hit("bcast_add_bwd_mask_site")
            if (int(a[4]) - c.site) % 8 == 5:
                self.hit("bcast_add_bwd_label")
        elif name == "layernorm_bwd":
            if kw.get("masked") is not None:
                self.hit("ln_bwd_masked")
            if c.live is not None:
                self.hit("ln_bwd_prefix_only" if a[0].shape[0] == c.live[1] else "ln_bwd_full")

    def __enter__(self):
        import deepsvg_amd.ops as ops
        for name in self.NAMES:
            fn = getattr(ops, name, None)
            if fn is None:
                continue
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name, **kw):
                ret = _fn(*a, **kw)
                self._note(_name, a, kw, ret)
                return ret
            setattr(ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        import deepsvg_amd.ops as ops
        for name, fn in self.saved.items():
            setattr(ops, name, fn)

    def check(self, on_gpu):
        for key, want in self.case.expect.items():
            if key.startswith("gpu:"):
                if not on_gpu:
                    continue
                key = key[4:]
            got = self.n.get(key, 0)
            assert (got > 0) if want == ">0" else (got == want), \
                f"{self.case.id}: route not taken - {key} ran {got} times, expected {want}; all counts {self.n}"


def _cfg_for(kind):
    from tests import helpers as H
    from tests import long_ops_ref as LR
    cfg = LR.long_cfg(126) if kind == "long126" else H.build_cfg(kind)
    cfg.dropout = DROP_P
    return cfg


def _patch_routes(monkeypatch, min_rows=None, gs_stack=True, ln_masked=True):
    import deepsvg_amd.functional as Fn
    if min_rows is not None:
        monkeypatch.setattr(Fn, "FFN_MIN_ROWS", min_rows)
        monkeypatch.setattr(Fn, "ATTN_MIN_ROWS", min_rows)
    else:
        monkeypatch.setattr(Fn, "FFN_MIN_ROWS", 16384)
        monkeypatch.setattr(Fn, "ATTN_MIN_ROWS", 16384)
    monkeypatch.setattr(Fn, "GS_STACK", gs_stack)
    monkeypatch.setattr(Fn, "LN_BWD_MASKED", ln_masked)
    monkeypatch.setattr(Fn, "GS_REMAINDER", 512)
    monkeypatch.setattr(Fn, "FFN_GATE_DW2", True)
    monkeypatch.setattr(Fn, "DEFER_MORE", True)


def _train_model(cfg, device, dtype, wseed):
    import deepsvg_amd
    from tests import helpers as H
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(H.weights_for(model, wseed))
    model.to(device)
    model.set_compute_dtype(dtype)
    model.train()
    model._own_seed = False         # the frozen seed: every run of the case draws the same masks
    model._seed = torch.tensor([SEED], dtype=torch.int64, device=device)
    return model


def run_stack_case(case, device, monkeypatch, on_gpu=False):
    """one _run_stack call + backward with whatever `ops` holds -> (results on the CPU, reference parameters, inputs)"""
    import deepsvg_amd.ops as ops
    cfg = _cfg_for(case.kind)
    if hasattr(cfg, "n_layers"):
        cfg.n_layers = cfg.n_layers_decode = case.n_layers
    _patch_routes(monkeypatch, case.min_rows, case.gs_stack, case.ln_masked)
    device = torch.empty(0, device=device).device
    dtype = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    model = _train_model(cfg, device, dtype, 31)
    model.hoist_global = case.hoist
    stack = model
    for part in case.stack.split("."):
        stack = getattr(stack, part)
    assert len(stack.layers) == case.n_layers
    inp = make_inputs(case, dim_z=cfg.dim_z, dim_label=getattr(cfg, "dim_label", 64))
    dev = {k: v.to(device=device, dtype=dtype).clone() for k, v in inp.items()}
    x = dev["x"].requires_grad_()
    z = dev["z"].requires_grad_() if case.z else None
    l = dev["l"].requires_grad_() if case.l else None
    key_mask = seq_off = tiles = None
    if case.key_bits is not None:
        key_mask = torch.tensor(case.key_bits, dtype=torch.int64, device=device)
    elif case.key_lens is not None:
        key_mask = torch.tensor(case.key_lens, dtype=torch.int32, device=device)
    with _Counters(case) as cnt:
        rt = model._runtime(device)
        rt.path_stage = case.path_stage
        if case.packed_lens is not None:
            off = [0]
            for n in case.packed_lens:
                off.append(off[-1] + n)
            seq_off = torch.tensor(off, dtype=torch.int32, device=device)
            tiles = ops.attention_tiles(seq_off, case.n_seq)
        out = model._run_stack(rt, stack, x, key_mask, z, case.n_seq, case.S, case.site, seq_off=seq_off, live=case.live,
                               tiles=tiles, l=l, causal=case.causal)
        out.backward(dev["dout"])
        if device.type == "cuda":
            torch.cuda.synchronize()
    cnt.check(on_gpu)
    res = {"out": out.detach(), "dx": x.grad}
    if z is not None:
        res["dz"] = z.grad
    if l is not None:
        res["dl"] = l.grad
    params = {}
    for name, prm in stack.named_parameters():
        if prm.grad is not None:
            res["grad:" + name] = prm.grad
        params[name] = (rt.w(prm) if prm.dim() >= 2 else prm).detach().double().cpu()
    return {k: v.detach().float().cpu() for k, v in res.items()}, params, inp


def seed_tensor():
    return torch.tensor([SEED], dtype=torch.int64)


def reference_for(case, params, inp, wrong_site=None):
    return stack_reference(case, params, inp["x"], inp.get("z"), inp.get("l"), inp["dout"], seed_tensor(), wrong_site)


@contextlib.contextmanager
def emulated(long_paths=False):
    """the restatements in place of `ops` for the length of the block (what the emulated_ops fixture does for a whole test)"""
    from tests import long_ops_ref as LR
    from tests.conftest import install_emulated_ops, restore_ops
    saved = install_emulated_ops()
    saved_long = LR.install() if long_paths else None
    try:
        yield
    finally:
        if saved_long is not None:
            LR.restore(saved_long)
        restore_ops(saved)


def parity_log(name, line):
    """print the line; with DSVG_PARITY_LOG_DIR set, also append it to `name` in that directory (how profiles/*.log are taken)"""
    print(line)
    out_dir = os.environ.get("DSVG_PARITY_LOG_DIR")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, name), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


# ----------------------------------------------------------------------------------------------------
# the dropout front ends: EmbedFn (sites 1), PackedEmbedFn (site 1), AddPosFn (sites 2 and 4)
# ----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class FrontCase:
    name: str
    dtype: str
    fn: str                         # "embed" | "packed" | "addpos"
    kind: str
    module: str                     # attribute path of the embedding / position table module
    n_seq: int
    S: int
    site: int
    group: bool = False             # EmbedFn with the group table (one-stage encoder)
    with_x: bool = False            # AddPosFn with an input (else the constant embedding)
    live: tuple = None
    packed_lens: list = None        # (PackedEmbedFn: every row is compared, the inert ones included)
    rows: int = None

    @property
    def id(self):
        return f"{self.name}-{self.dtype}"

    def sites(self):
        return [self.site]


def _front_cases():
    c = []
    for dt in ("fp32", "bf16"):
        c.append(FrontCase("embed", dt, "embed", "hier", "encoder.embedding", 6, 30, 1))
        c.append(FrontCase("embed_group", dt, "embed", "onestage", "encoder.embedding", 4, 40, 1, group=True))
        c.append(FrontCase("packed_embed", dt, "packed", "hier", "encoder.embedding", 30, 30, 1, rows=512))
        c.append(FrontCase("add_pos_x", dt, "addpos", "hier", "encoder.hierarchical_PE", 16, 8, 2, with_x=True))
        c.append(FrontCase("add_pos_const_live", dt, "addpos", "hier", "decoder.embedding.PE", 6, 30, 4, live=(3, 128)))
    return c


FRONT_CASES = _front_cases()


def _front_inputs(case, cfg, n_group_rows):
    g = torch.Generator().manual_seed(77)
    rows = case.rows or case.n_seq * case.S
    t = {"dout": torch.randn(rows, 256, generator=g)}
    if case.fn != "addpos":
        t["commands"] = torch.randint(0, cfg.n_commands, (rows,), generator=g).float()
        t["args"] = torch.randint(-1, cfg.args_dim, (rows, cfg.n_args), generator=g).float()
        if case.group:
            t["groups"] = torch.randint(0, n_group_rows, (rows,), generator=g).to(torch.int32)
        if case.fn == "packed":     # lengths 1 .. 30 back to back, then inert rows that replicate token 0
            lens = list(range(1, case.n_seq + 1))
            pos = torch.cat([torch.arange(n) for n in lens])
            t["pos_idx"] = torch.cat([pos, torch.zeros(rows - pos.numel(), dtype=pos.dtype)]).to(torch.int32)
    elif case.with_x:
        t["x"] = torch.randn(rows, 256, generator=g)
    if case.live is not None:
        t["dout"][case.live[0] * case.S:] = 0
    if case.dtype == "bf16":
        t = {k: (v.to(torch.bfloat16).float() if k in ("dout", "x") else v) for k, v in t.items()}
    return t


def front_reference(case, params, inp, seed, wrong_site=None):
    """float64 autograd over drop(embed_fcn(arg_embed[args + 1]) + command_embed[cmd] (+ group | pos) + pos) resp. drop(x + pos);
    the mask ids are those of R.add_pos_fwd / R.gemm: element (row, column) of the [rows, 256] result"""
    from deepsvg_amd.model import PE_DROPOUT
    site = case.site + WRONG if wrong_site == case.site else case.site
    P = {k: v.detach().double().cpu().clone().requires_grad_() for k, v in params.items()}
    rows = inp["dout"].shape[0]
    x = None
    if case.fn == "addpos":
        v = P["pos"][:case.S].repeat(case.n_seq, 1)
        if case.with_x:
            x = inp["x"].detach().double().clone().requires_grad_()
            v = v + x
    else:
        a = (inp["args"].long() + 1).clamp(0, P["arg"].shape[0] - 1)
        v = P["arg"][a].reshape(rows, -1) @ P["fcn_w"].t() + P["fcn_b"] + P["cmd"][inp["commands"].long()]
        if case.group:
            v = v + P["grp"][inp["groups"].long()]
        if case.fn == "packed":
            v = v + P["pos"][:case.S][inp["pos_idx"].long()]
        else:
            v = v + P["pos"][:case.S].repeat(case.n_seq, 1)
    out = v * R.drop_mult(PE_DROPOUT, seed, site, R._ids(rows, 256, v.device)).double()
    out.backward(inp["dout"].double())
    res = {"out": out.detach()}
    if x is not None:
        res["dx"] = x.grad
    for k, prm in P.items():
        res["grad:" + k] = prm.grad if prm.grad is not None else torch.zeros_like(prm)
    return res


def run_front_case(case, device, monkeypatch, on_gpu=False):
    """one front-end Function + backward with whatever `ops` holds -> (results on the CPU, reference parameters, inputs)"""
    import deepsvg_amd.functional as Fn
    from deepsvg_amd.model import PE_DROPOUT
    cfg = _cfg_for(case.kind)
    cfg.n_layers = cfg.n_layers_decode = 1
    _patch_routes(monkeypatch)
    device = torch.empty(0, device=device).device
    dtype = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    model = _train_model(cfg, device, dtype, 32)
    mod = model
    for part in case.module.split("."):
        mod = getattr(mod, part)
    if case.fn == "addpos":
        tabs = {"pos": mod.pos_embed.weight}
    else:
        tabs = {"cmd": mod.command_embed.weight, "arg": mod.arg_embed.weight, "fcn_w": mod.embed_fcn.weight,
                "fcn_b": mod.embed_fcn.bias, "pos": mod.pos_encoding.pos_embed.weight}
        if case.group:
            tabs["grp"] = mod.group_embed.weight
    inp = _front_inputs(case, cfg, tabs["grp"].shape[0] if case.group else 0)
    dev = {k: (v.to(device=device, dtype=dtype).clone() if k in ("dout", "x") else v.to(device)) for k, v in inp.items()}
    x = dev["x"].requires_grad_() if "x" in dev else None
    with _Counters(case) as cnt:
        rt = model._runtime(device)
        if case.fn == "embed":
            out = Fn.EmbedFn.apply(rt, dev["commands"], dev["args"], dev.get("groups"), case.n_seq, case.S, PE_DROPOUT, case.site,
                                   tabs["cmd"], tabs["arg"], tabs["fcn_w"], tabs["fcn_b"], tabs["pos"], tabs.get("grp"))
        elif case.fn == "packed":
            out = Fn.PackedEmbedFn.apply(rt, dev["commands"], dev["args"], dev["pos_idx"], case.S, PE_DROPOUT, case.site,
                                         tabs["cmd"], tabs["arg"], tabs["fcn_w"], tabs["fcn_b"], tabs["pos"])
        else:
            out = Fn.AddPosFn.apply(rt, x, tabs["pos"], case.n_seq, case.S, PE_DROPOUT, case.site, case.live)
        out.backward(dev["dout"])
        if device.type == "cuda":
            torch.cuda.synchronize()
    want = {"embed": ("embed_gather", "add_pos_fwd", "add_pos_bwd", "embed_scatter"),
            "packed": ("embed_gather", "drop_apply", "embed_scatter"), "addpos": ("add_pos_fwd", "add_pos_bwd")}[case.fn]
    assert all(cnt.n.get(k, 0) > 0 for k in want), (case.id, cnt.n)
    res = {"out": out.detach()}
    if x is not None:
        res["dx"] = x.grad
    params = {}
    for k, prm in tabs.items():
        res["grad:" + k] = prm.grad
        # the reference multiplies with what the product multiplies with: the bf16 images of the tables and of the matrix in a
        # bf16 run (the gather rounds a table row as the image does); the position table is added in fp32
        lp = dtype == torch.bfloat16 and prm.dim() >= 2 and k != "pos"
        params[k] = (prm.detach().to(torch.bfloat16) if lp else prm.detach()).double().cpu()
    return {k: v.detach().float().cpu() for k, v in res.items()}, params, inp
