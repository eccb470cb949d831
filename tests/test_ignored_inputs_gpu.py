"""Kernel contracts at the level of one `ops` call (the C ABI of include/dsvg.h that external callers use): what a kernel is
meant to ignore, it ignores.  Every case runs the same call twice - the ignored region zero, then poisoned - and the defined
part of every output must be bit-equal (`torch.equal`); regions a kernel promises to clear must be exactly 0, and memory
around an output view must be left as it was.  Two poison strengths, by what the region's contract supports:

  * OUTSIDE any sequence or matrix (bucket rows behind seq_off[n_seq], rows behind M of a larger allocation, columns between
    the logical width and the row stride): NaN.  Nothing may read them into a result - a tile that multiplies by 0 instead
    of selecting shows up as NaN.
  * INSIDE the layout but masked (K / V rows of masked keys, a neighbouring sequence in the same tile, weight-0 tokens):
    finite garbage, 1e3 * randn rounded to the storage type.  NaN there is legitimately contagious through 0 * NaN in an
    MFMA, and the reference behaves the same within a sample.

The poisoned run also allocates under `poisoned_empty(NaN)` (tests/poison.py), so that every output buffer and workspace the
op makes for itself is born as NaN: a region a kernel promises to clear and does not, or a workspace it reads before writing,
shows up whatever the allocator happened to hand back.

No index, offset, length or mask is ever poisoned: integer inputs are the same valid values in both runs."""
import contextlib

import pytest
import torch

from deepsvg_amd import ops
from tests import test_group_stage_gpu as GS
from tests.poison import poisoned_empty
from tests.test_kernels_gpu import _attn_setup, _rand, _seed_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DTYPES = [torch.float32, torch.bfloat16]
SCALE = 32 ** -0.5


def _garbage(*shape, dtype, seed):
    return _rand(*shape, dtype=torch.float32, seed=seed, scale=1e3).to(dtype)


def _up8(n):
    return (n + 7) // 8 * 8


def _all_nan(t):
    return t.numel() == 0 or bool(torch.isnan(t).all())


def _filled(t, fill):
    return _all_nan(t) if fill != fill else bool((t == fill).all())


def _born_nan(on=True):
    """the allocations of the poisoned run"""
    return poisoned_empty(NAN) if on else contextlib.nullcontext()


def _eq(clean, dirty, what=""):
    """dicts (or sequences) of tensors: same dtype, finite, and the same bits"""
    if not isinstance(clean, dict):
        clean, dirty = dict(enumerate(clean)), dict(enumerate(dirty))
    assert clean.keys() == dirty.keys()
    for k, c in clean.items():
        d = dirty[k]
        assert c.dtype == d.dtype and c.shape == d.shape, (what, k)
        assert not c.is_floating_point() or bool(torch.isfinite(c.float()).all()), f"{what} {k}: the clean run is not finite"
        if not torch.equal(c, d):
            bad = (c != d) | (d != d)
            raise AssertionError(f"{what} {k}: {int(bad.sum())} of {c.numel()} elements differ with the ignored region poisoned "
                                 f"({int((d != d).sum())} NaN), first at flat index {int(bad.reshape(-1).nonzero()[0])}")


# ---- GEMM family -----------------------------------------------------------------------------------------------------------
def _operand(rows, cols, dtype, seed, fill, extra_rows=5, pad=8):
    """a [rows, cols] leading view of a [rows + extra_rows, up8(cols) + pad] buffer whose other elements hold `fill`"""
    buf = torch.full((rows + extra_rows, _up8(cols) + pad), fill, dtype=dtype, device=DEV)
    buf[:rows, :cols] = _rand(rows, cols, dtype=dtype, seed=seed)
    return buf[:rows, :cols]


def _gemm_case(dtype, impl, M, N, K, a_kc, b_kc, fill):
    a = _operand(*((M, K) if a_kc else (K, M)), dtype, 1, fill)
    b = _operand(*((N, K) if b_kc else (K, N)), dtype, 2, fill)
    bias = _rand(N, seed=3)
    obuf = torch.full((M + 3, _up8(N) + 8), fill, dtype=dtype, device=DEV)
    with _born_nan(fill != fill):
        ops.gemm(a, b, a_kc=a_kc, b_kc=b_kc, bias=bias, out=obuf[:M, :N], impl=impl)
    torch.cuda.synchronize()
    assert _filled(obuf[M:], fill) and _filled(obuf[:M, N:], fill), "wrote outside the output view"
    return obuf[:M, :N].clone()


@pytest.mark.parametrize("dtype,impl", [(torch.float32, 0), (torch.float32, 1), (torch.bfloat16, 0), (torch.bfloat16, 1),
                                        (torch.bfloat16, 2), (torch.bfloat16, 3), (torch.bfloat16, 4), (torch.bfloat16, 6)])
def test_gemm_reads_nothing_behind_its_operands(gpu_device, dtype, impl):
    """operands are leading-row views of buffers whose remaining rows and row padding are NaN, the output a view of a NaN
    buffer: the K tail, the M / N tails and the row padding are selected away, never multiplied; all four layouts.  The
    LDS-DMA variants (impl 3 / 4 / 6: 2, 1 and 4 stages; impl 0 tries them first) take k-contiguous A with K a multiple of 64
    and hand everything else to the register-staged kernel (impl 2): K = 64 is one K step, 520 x 264 x 1024 sixteen - the
    pipelines of every depth fill, run and drain - and K = 1000 is the K tail of the register-staged kernel"""
    for M, N, K in [(129, 8, 64), (300, 200, 64), (520, 264, 1000), (520, 264, 1024)]:
        for a_kc in (True, False):
            for b_kc in (True, False):
                clean, dirty = (_gemm_case(dtype, impl, M, N, K, a_kc, b_kc, f) for f in (0.0, NAN))
                assert clean.abs().max() > 0
                _eq([clean], [dirty], f"gemm {M}x{N}x{K} a_kc={a_kc} b_kc={b_kc} impl={impl} {dtype}")


def _wgrad_case(dtype, impl, T, n_out, k_in, split, fill, rowsum, mode="immediate"):
    """dW [n_out, k_in] (+ db) = the leading T rows of two token-major buffers that hold `fill` in 37 more rows and in their
    row padding (dy: up8(n_out) columns, as the model's buffers - 523 in 528; x: 8 more)"""
    dy, x = _operand(T, n_out, dtype, 21, fill, extra_rows=37, pad=0), _operand(T, k_in, dtype, 22, fill, extra_rows=37)
    flat = torch.full((n_out * k_in + n_out + 64,), fill, dtype=torch.float32, device=DEV)
    dw, db = flat[:n_out * k_in].view(n_out, k_in), flat[n_out * k_in:n_out * k_in + n_out]
    cs = torch.full((n_out + 8,), fill, dtype=torch.float32, device=DEV)
    with contextlib.ExitStack() as st:
        st.enter_context(_born_nan(fill != fill))           # the split-K slices and the column partials are born NaN
        if mode != "immediate":
            st.enter_context(ops.DEFER)
        if mode == "grouped":
            st.enter_context(ops.GROUP)
        ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=split, rowsum=db if rowsum else None, impl=impl)
        ops.colsum(dy, out=cs[:n_out])
    ops.flush_deferred()
    torch.cuda.synchronize()
    used = n_out * k_in + (n_out if rowsum else 0)
    assert _filled(flat[used:], fill) and _filled(cs[n_out:], fill), "wrote behind the gradient"
    return {"dw": dw.clone(), "db": db.clone() if rowsum else cs[:n_out].clone(), "colsum": cs[:n_out].clone()}


# T, n_out, k_in, split, and whether the LDS-DMA kernel takes the shape (csrc/gemm_bf16_glds.hip: K = T a multiple of 64, at
# least 8 output rows; a ragged n_out is fine)
WGRAD_SHAPES = [(640, 264, 704, 3, True),       # the LDS-DMA weight-gradient shape of test_kernels_gpu.py, 37 NaN rows behind it
                (640, 523, 256, 8, True),       # ragged M under its 8-element chunk reads (523 columns in 528), 3 empty K slices,
                                                # one grid plane: inside ops.GROUP the launch goes through the group queue
                (640 + 37, 264, 704, 3, False),  # K tail: the register-staged kernel
                (992, 7, 256, 4, False)]        # fewer than 8 output rows: the register-staged kernel


@pytest.mark.parametrize("T,n_out,k_in,split,lds_dma", WGRAD_SHAPES)
@pytest.mark.parametrize("dtype,impl", [(torch.float32, 0), (torch.bfloat16, 0), (torch.bfloat16, 2), (torch.bfloat16, 3),
                                        (torch.bfloat16, 4), (torch.bfloat16, 6)])
def test_weight_gradients_sum_over_their_rows_only(gpu_device, dtype, impl, T, n_out, k_in, split, lds_dma):
    """split-K weight gradients (token-major operands, the fused `rowsum` bias gradient, `colsum`) over the leading T rows of
    buffers whose later rows and row padding are NaN, into accumulators that hold NaN beforehand (accumulate=False), with
    split-K slices born NaN; immediately, inside a deferral scope, and queued in a group scope.  That impl 0 / 3 / 4 / 6
    really ran the LDS-DMA kernel where the shape allows it shows in the bits: it keeps its slices in bf16, the
    register-staged kernel (impl 2) in fp32"""
    for rowsum in (True, False):
        res = {}
        for mode in ("immediate", "deferred", "grouped"):
            clean, dirty = (_wgrad_case(dtype, impl, T, n_out, k_in, split, f, rowsum, mode) for f in (0.0, NAN))
            assert clean["dw"].abs().max() > 0 and clean["db"].abs().max() > 0
            _eq(clean, dirty, f"wgrad T={T} {n_out}x{k_in} split={split} impl={impl} rowsum={rowsum} {mode}")
            res[mode] = clean
        assert torch.equal(res["grouped"]["dw"], res["deferred"]["dw"])         # one launch for the group: the same bits
        if dtype == torch.bfloat16:
            staged = _wgrad_case(dtype, 2, T, n_out, k_in, split, 0.0, rowsum)
            assert torch.equal(res["immediate"]["dw"], staged["dw"]) == (impl == 2 or not lds_dma), \
                "the shape did not reach the kernel this case is about"


# ---- attention, packed layout ----------------------------------------------------------------------------------------------
def _packed_layout():
    """40 sequences of 1 .. 30 rows, several per 32-row tile; rows rounded up to 256, plus 64"""
    lens = torch.tensor([1 + (7 * i) % 30 for i in range(40)])
    lens[3], lens[4], lens[5] = 1, 2, 30
    off = torch.zeros(41, dtype=torch.int32)
    off[1:] = lens.cumsum(0)
    real = int(off[-1])
    rows = (real + 255) // 256 * 256 + 64
    seq = torch.repeat_interleave(torch.arange(40), lens)
    odd = torch.zeros(rows, dtype=torch.bool)
    odd[:real] = seq % 2 == 1
    even = torch.zeros(rows, dtype=torch.bool)
    even[:real] = seq % 2 == 0
    seq_off = off.to(DEV)
    return seq_off, ops.attention_tiles(seq_off, 40, 32), real, rows, odd.to(DEV), even.to(DEV)


def _packed_runs(mode):
    """every packed-layout attention entry point on one set of inputs.  mode 'clean'; 'nan': rows [real, rows) of qkv / x are
    NaN (their gradient rows stay 0: the caller's duty); 'odd': every odd sequence's rows hold finite garbage"""
    seq_off, tiles, real, rows, odd, _ = _packed_layout()
    flat, offs, prm = _attn_setup(seed=13)
    qkv = (_rand(rows, 768, seed=33) * 0.8).to(torch.bfloat16)
    x = (_rand(rows, 256, seed=32) * 1.5 + 0.3).to(torch.bfloat16)
    dout = (_rand(rows, 256, seed=34) * 0.6).to(torch.bfloat16)
    dout[real:] = 0
    for t in (qkv, x):
        t[real:] = 0
    if mode == "nan":
        qkv[real:] = NAN
        x[real:] = NAN
    elif mode == "odd":
        qkv[odd] = _garbage(rows, 768, dtype=torch.bfloat16, seed=35)[odd]
        x[odd] = _garbage(rows, 256, dtype=torch.bfloat16, seed=36)[odd]
        dout[odd] = _garbage(rows, 256, dtype=torch.bfloat16, seed=37)[odd]
    seed = _seed_tensor(0x0BADC0FFEE12345B)
    wob = ops.attn_pack_bwd(flat, offs, 2)[ops.ATTN_BWD_LAYER_ELEMS:2 * ops.ATTN_BWD_LAYER_ELEMS]
    packed = ops.attn_pack(flat, offs, 2)[:ops.ATTN_LAYER_ELEMS]
    out = {}
    for name, tl in (("", None), ("/tiles", tiles)):
        out["fwd" + name] = ops.attention_fwd(qkv, None, 40, 30, 8, SCALE, 0.1, 7, seed, seq_off=seq_off, tiles=tl)
        out["bwd" + name] = ops.attention_bwd(qkv, None, dout, 40, 30, 8, SCALE, 0.1, 7, seed, seq_off=seq_off, tiles=tl)
    out["bwd_outproj"] = ops.attention_bwd_outproj(qkv, None, dout, wob, 40, 30, SCALE, 0.1, 7, seed, seq_off=seq_off, tiles=tiles)
    blk = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], None, 40, 30, SCALE, 1e-5,
                             0.1, 7, 8, seed, seq_off=seq_off, tiles=tiles, train=True)
    for n, t in zip(("x1", "xn", "qkv", "ao", "mean", "rstd"), blk):
        out["block/" + n] = t
    out["block/x1_inference"] = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], None, 40,
                                                   30, SCALE, 1e-5, 0.1, 7, 8, seed, seq_off=seq_off, tiles=tiles)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def packed_clean(gpu_device):
    return _packed_runs("clean")


def test_packed_attention_ignores_the_bucket_rows(gpu_device, packed_clean):
    """NaN in the rows behind the last sequence: rows [:real] bit-equal; rows [real:] of the outputs whose tail workgroup
    clears them (attention_fwd / attention_bwd / attention_bwd_outproj) exactly 0.  attn_block_fwd computes its bucket rows from
    themselves alone (include/dsvg.h: they attend to themselves only): they are compared nowhere"""
    _, _, real, rows, _, _ = _packed_layout()
    with _born_nan():
        dirty = _packed_runs("nan")
    _eq({k: v[:real] for k, v in packed_clean.items()}, {k: v[:real] for k, v in dirty.items()}, "packed attention, NaN bucket rows")
    for k, v in dirty.items():
        if not k.startswith("block/"):
            assert v.shape[0] == rows and torch.count_nonzero(v[real:]) == 0, f"{k}: rows behind the last sequence are not 0"
            assert torch.count_nonzero(packed_clean[k][real:]) == 0, k


def test_packed_attention_isolates_the_sequences_of_a_tile(gpu_device, packed_clean):
    """finite garbage in every odd sequence: the even sequences' rows are bit-equal (block-diagonal attention inside a tile)"""
    even = _packed_layout()[5]
    with _born_nan():
        dirty = _packed_runs("odd")
    _eq({k: v[even] for k, v in packed_clean.items()}, {k: v[even] for k, v in dirty.items()}, "packed attention, garbage neighbours")
    assert any(not torch.equal(packed_clean[k], dirty[k]) for k in dirty)           # the garbage was read by its own sequences


# ---- attention, dense layouts with a key mask ------------------------------------------------------------------------------
N_SEQ = 12


def _valid_keys(S, arbitrary):
    """bool [12, S]: one sequence with a single visible key, one full; every sequence has at least one"""
    g = torch.Generator().manual_seed(S)
    if arbitrary:
        bits = torch.rand(N_SEQ, S, generator=g) < 0.5
        bits[torch.arange(N_SEQ), torch.randint(0, S, (N_SEQ,), generator=g)] = True
        bits[0] = False
        bits[0, S // 2] = True
    else:
        lens = torch.randint(1, S + 1, (N_SEQ,), generator=g)
        lens[0] = 1
        bits = torch.arange(S).unsqueeze(0) < lens.unsqueeze(1)
    bits[1] = True
    return bits


def _key_mask(valid, S):
    if S > 64:
        return valid.sum(1).to(torch.int32).to(DEV)                 # valid-prefix lengths
    return (valid.to(torch.int64) << torch.arange(S, dtype=torch.int64)).sum(1).to(DEV)


def _dense_attention(dtype, S, causal, path_stage, arbitrary, garbage):
    valid = _valid_keys(S, arbitrary)
    km = _key_mask(valid, S)
    dead = (~valid).reshape(-1).to(DEV)
    qkv = _rand(N_SEQ * S, 768, dtype=dtype, seed=S)
    if garbage:
        qkv[dead, 256:] = _garbage(N_SEQ * S, 512, dtype=dtype, seed=S + 1)[dead]
    do = _rand(N_SEQ * S, 256, dtype=dtype, seed=S + 2)
    seed = _seed_tensor(0x0123456789ABCDEF)
    out = ops.attention_fwd(qkv, km, N_SEQ, S, 8, SCALE, 0.1, 21, seed, causal=causal, path_stage=path_stage)
    dqkv = ops.attention_bwd(qkv, km, do, N_SEQ, S, 8, SCALE, 0.1, 21, seed, causal=causal, path_stage=path_stage)
    torch.cuda.synchronize()
    assert torch.count_nonzero(dqkv[dead, 256:]) == 0, "dk / dv of a masked key is not exactly 0"
    return {"out": out, "dq": dqkv[:, :256].clone(), "dkv": dqkv[~dead, 256:].clone()}


@pytest.mark.parametrize("dtype,S,causal,path_stage,arbitrary", [
    (torch.float32, 8, False, False, True), (torch.float32, 31, False, False, False),      # attention.hip
    (torch.bfloat16, 32, False, False, False), (torch.bfloat16, 8, False, False, True),    # attention_mfma.hip: one / four sequences per tile
    (torch.float32, 65, False, False, False), (torch.bfloat16, 102, False, False, False),  # long_seq.hip
    (torch.bfloat16, 65, False, True, False), (torch.bfloat16, 102, False, True, False),   # attention_long_mfma.hip
    (torch.float32, 102, False, True, False),                                              # the padded long route
    (torch.float32, 31, True, False, False), (torch.bfloat16, 31, True, False, False),     # causal
    (torch.bfloat16, 102, True, False, False)])
def test_dense_attention_ignores_masked_keys(gpu_device, dtype, S, causal, path_stage, arbitrary):
    """finite garbage in K and V at masked positions only: the output at all rows, dq everywhere and dk / dv at valid keys are
    bit-equal; dk / dv at masked keys are exactly 0"""
    clean = _dense_attention(dtype, S, causal, path_stage, arbitrary, False)
    with _born_nan():
        dirty = _dense_attention(dtype, S, causal, path_stage, arbitrary, True)
    _eq(clean, dirty, f"attention S={S} {dtype} causal={causal} path_stage={path_stage}")


def _gs_inputs():
    n_seq, S = 13, 8                                        # four sequences per tile, one in the last
    flat, offs, p, x, km, seq_add, dx2 = GS._setup(n_seq, S, seed=5, masked=True, with_add=True)
    pf, pb = ops.gs_pack(flat, offs, 2)
    valid = ((km.unsqueeze(1) >> torch.arange(S, device=DEV)) & 1).bool().reshape(-1)
    xg = x.clone()
    xg[~valid] = _garbage(n_seq * S, 256, dtype=torch.bfloat16, seed=6)[~valid]
    return n_seq, S, p, x, xg, km, seq_add, dx2, pf, pb, valid


def _poison_kv(qkv, valid):
    q = qkv.clone()
    q[~valid, 256:] = _garbage(qkv.shape[0], 512, dtype=torch.bfloat16, seed=7)[~valid]
    return q


def _check_gs_bwd(clean, dirty, valid, what):
    """(dx, dym, dpre, dx1m, dqkv, dgamma2, dbeta2, dgamma1, dbeta1[, dg ...]) of a run on the saved q|k|v and of one with garbage
    in its K / V rows of masked keys"""
    for t in (clean["dqkv"], dirty["dqkv"]):
        assert torch.count_nonzero(t[~valid, 256:]) == 0, f"{what}: dk / dv of a masked key is not exactly 0"
    _eq(clean, dirty, what)


def test_group_stage_layer_ignores_masked_keys(gpu_device):
    """gs_layer_fwd with garbage in the rows of x whose key is masked: every output row of a visible position is bit-equal.
    gs_layer_bwd with garbage in K and V of the saved q|k|v at masked keys: every result is bit-equal, dk / dv there exactly 0;
    its four LayerNorm gradient outputs are handed over holding NaN"""
    n_seq, S, p, x, xg, km, seq_add, dx2, pf, pb, valid = _gs_inputs()
    seed = _seed_tensor(0x0123456789ABCDEF)
    sl = slice(0, ops.GS_LAYER_ELEMS)
    fwd = lambda xx: ops.gs_layer_fwd(xx, pf[sl], *GS._params(p), km, n_seq, S, SCALE, 1e-5, 0.1, 300, seed, seq_add=seq_add, train=True)
    clean = fwd(x)
    with _born_nan():
        dirty = fwd(xg)
    _eq({n: t[valid] for n, t in zip(GS.FWD_NAMES, clean)}, {n: t[valid] for n, t in zip(GS.FWD_NAMES, dirty)}, "gs_layer_fwd")
    sv = dict(zip(GS.FWD_NAMES, clean))

    def bwd(qkv, fill):
        acc = [torch.full((256,), fill, device=DEV) for _ in range(4)]
        with _born_nan(fill != fill):
            r = ops.gs_layer_bwd(dx2, pb[sl], x, sv["mean1"], sv["rstd1"], qkv, sv["x1"], sv["mean2"], sv["rstd2"], sv["h"], p["gamma1"],
                                 p["gamma2"], km, n_seq, S, SCALE, 0.1, 300, seed, want_dx1=True, dgamma2=acc[0], dbeta2=acc[1],
                                 dgamma1=acc[2], dbeta1=acc[3], want_dg=True)
        torch.cuda.synchronize()
        return dict(zip(GS.BWD_NAMES + ("dg",), r))
    _check_gs_bwd(bwd(sv["qkv"], 0.0), bwd(_poison_kv(sv["qkv"], valid), NAN), valid, "gs_layer_bwd")


def test_group_stage_stack_ignores_masked_keys(gpu_device):
    """the same through gs_stack_fwd / gs_stack_bwd, two layers in one launch"""
    n_seq, S, p, x, xg, km, seq_add, dx2, pf, pb, valid = _gs_inputs()
    seed = _seed_tensor(0x0123456789ABCDEF)
    E = ops.GS_LAYER_ELEMS
    names = ("in_bias", "out_bias", "b1", "b2", "gamma1", "beta1", "gamma2", "beta2")
    layers = [dict(img=pf[i * E:(i + 1) * E], site0=300 + 8 * i, seq_add=seq_add, **{k: p[k] for k in names}) for i in range(2)]
    fwd = lambda xx: ops.gs_stack_fwd(xx, layers, km, n_seq, S, SCALE, 1e-5, 0.1, seed, train=True)
    clean = fwd(x)
    with _born_nan():
        dirty = fwd(xg)
    for i in range(2):
        _eq({n: t[valid] for n, t in zip(GS.FWD_NAMES, clean[i])}, {n: t[valid] for n, t in zip(GS.FWD_NAMES, dirty[i])},
            f"gs_stack_fwd layer {i}")
    assert torch.equal(ops.gs_stack_fwd(xg, layers, km, n_seq, S, SCALE, 1e-5, 0.1, seed)[1][valid], clean[1][0][valid])

    def bwd(poison, fill):
        bl, accs = [], []
        for i in range(2):
            sv = dict(zip(GS.FWD_NAMES, clean[i]))
            acc = {k: torch.full((256,), fill, device=DEV) for k in ("dgamma2", "dbeta2", "dgamma1", "dbeta1")}
            accs.append(acc)
            bl.append(dict(img=pb[i * E:(i + 1) * E], x=x if i == 0 else clean[0][0], mean1=sv["mean1"], rstd1=sv["rstd1"],
                           qkv=_poison_kv(sv["qkv"], valid) if poison else sv["qkv"], x1=sv["x1"], mean2=sv["mean2"],
                           rstd2=sv["rstd2"], h=sv["h"], gamma1=p["gamma1"], gamma2=p["gamma2"], site0=300 + 8 * i, **acc))
        with _born_nan(poison):
            dx, per, dgcat = ops.gs_stack_bwd(dx2, bl, km, n_seq, S, SCALE, 0.1, seed, want_dg=True)
        torch.cuda.synchronize()
        res = []
        for i in range(2):
            r = dict(zip(("dym", "dpre", "dx1m", "dqkv"), per[i]))
            r.update(accs[i])
            res.append(r)
        res[0]["dx"], res[0]["dgcat"] = dx, dgcat
        return res
    c, d = bwd(False, 0.0), bwd(True, NAN)
    for i in range(2):
        _check_gs_bwd(c[i], d[i], valid, f"gs_stack_bwd layer {i}")


# ---- ld-padded logits and weight-0 tokens ----------------------------------------------------------------------------------
def _padded_logits(T, width, ld, dtype, seed, fill):
    buf = torch.full((T, ld), fill, dtype=dtype, device=DEV)
    buf[:, :width] = _rand(T, width, dtype=dtype, seed=seed, scale=2.0)
    return buf[:, :width]


def _ce_case(dtype, C_, group, ld, fill):
    T = 64
    g = torch.Generator().manual_seed(C_)
    logits = _padded_logits(T, group * C_, ld, dtype, 1, fill)
    target = torch.randint(0, C_, (T * group,), generator=g).to(torch.int32).to(DEV)
    w = (torch.rand(T * group, generator=g) < 0.6).float().to(DEV)
    lse, sc = ops.masked_ce_fwd(logits, target, w, C_, group)
    d = ops.masked_ce_bwd(logits, target, w, lse, sc, torch.tensor([0.7], device=DEV), 2.0, C_, group, pad_to=8)
    full = d.as_strided((T, d.stride(0)), (d.stride(0), 1))
    res = {"lse": lse, "sum_count": sc, "dlogits": d.clone(), "argmax": ops.argmax_rows(logits, C_, group),
           "sample": ops.sample_rows(logits, C_, 0.7, _seed_tensor(99), ops.SITE_SAMPLE_ARGS, group)}
    torch.cuda.synchronize()
    assert d.stride(0) % 8 == 0 and torch.count_nonzero(full[:, group * C_:]) == 0, "masked_ce_bwd: its own pad columns are not 0"
    assert int(res["argmax"].min()) >= 0 and int(res["argmax"].max()) < C_ and int(res["sample"].min()) >= 0 \
        and int(res["sample"].max()) < C_
    return res


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C_,group,ld", [(257, 11, 2832), (7, 1, 8)])
def test_loss_and_sampling_kernels_ignore_the_row_padding(gpu_device, dtype, C_, group, ld):
    """64 tokens in a buffer of row stride `ld`, viewed as [:, :group * C]: NaN in the pad columns"""
    clean = _ce_case(dtype, C_, group, ld, 0.0)
    with _born_nan():
        dirty = _ce_case(dtype, C_, group, ld, NAN)
    _eq(clean, dirty, f"ld-padded logits C={C_} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_ce_ignores_the_logits_of_weight_0_slots(gpu_device, dtype):
    """finite garbage in the logits of every (token, slot) whose weight is 0: sum / count, lse and dlogits at live slots
    bit-equal, dlogits at dead slots exactly 0"""
    T, C_, group = 64, 257, 11
    g = torch.Generator().manual_seed(8)
    target = torch.randint(0, C_, (T * group,), generator=g).to(torch.int32).to(DEV)
    w = (torch.rand(T, group, generator=g) < 0.4).float()
    w[torch.rand(T, generator=g) < 0.5] = 0.0                   # whole tokens without loss
    w = w.view(-1).to(DEV)
    live = w > 0
    res = []
    for garbage in (False, True):
        logits = _padded_logits(T, group * C_, 2832, dtype, 2, 0.0)
        if garbage:
            dead_cols = (~live).view(T, group).repeat_interleave(C_, dim=1)
            logits[dead_cols] = _garbage(T, group * C_, dtype=dtype, seed=3)[dead_cols]
        with _born_nan(garbage):
            lse, sc = ops.masked_ce_fwd(logits, target, w, C_, group)
            d = ops.masked_ce_bwd(logits, target, w, lse, sc, torch.tensor([0.7], device=DEV), 2.0, C_, group, pad_to=8)
        torch.cuda.synchronize()
        dv = d.reshape(T * group, C_)
        assert torch.count_nonzero(dv[~live]) == 0, "dlogits of a weight-0 slot is not exactly 0"
        res.append({"sum_count": sc, "lse": lse[live].clone(), "dlogits": dv[live].clone()})
    assert int(live.sum()) > 0 and res[0]["dlogits"].abs().max() > 0
    _eq(res[0], res[1], f"weight-0 slots {dtype}")


@pytest.mark.parametrize("group", [11, 6])
def test_fused_head_ignores_rows_without_loss(gpu_device, group):
    """head_lse / head_dlogits on the compact token list: finite garbage in the rows of x whose tok_idx entry is negative
    (padding of the list) and in the listed tokens without any weight"""
    C_, n_tok, rows = 257, 200, 128
    n_out = group * C_
    g = torch.Generator().manual_seed(group)
    target = torch.randint(0, C_, (n_tok * group,), generator=g).to(torch.int32).to(DEV)
    w = (torch.rand(n_tok, group, generator=g) < 0.5).float()
    w[torch.rand(n_tok, generator=g) < 0.4] = 0.0
    listed = torch.randperm(n_tok, generator=g)[:100].sort().values
    idx = torch.full((rows,), -1, dtype=torch.int32)
    idx[:100] = listed.to(torch.int32)
    idx[17] = -1                                                # a hole inside the list as well
    row_dead = (idx < 0) | (w.sum(1)[idx.clamp(min=0).long()] == 0)
    assert 0 < int(row_dead[:100].sum()) < 100
    idx, w, row_dead = idx.to(DEV), w.view(-1).to(DEV), row_dead.to(DEV)
    wt = _rand(n_out, 256, seed=4, scale=0.08, dtype=torch.bfloat16)
    b = _rand(n_out, seed=5, scale=0.5)
    img = ops.head_pack(wt)
    slot_live = (w.view(n_tok, group)[idx.clamp(min=0).long()] > 0) & (idx >= 0).unsqueeze(1)       # [rows, group]
    res = []
    for garbage in (False, True):
        x = _rand(rows, 256, seed=3, dtype=torch.bfloat16)
        if garbage:
            x[row_dead] = _garbage(rows, 256, dtype=torch.bfloat16, seed=6)[row_dead]
        with _born_nan(garbage):
            lse, sc = ops.head_lse(x, img, b, n_out, C_, target, w, tok_idx=idx)
            d = ops.head_dlogits(x, img, b, n_out, C_, target, w, lse, sc, torch.tensor([1.3], device=DEV), 1.0, tok_idx=idx)
        torch.cuda.synchronize()
        dv = d.reshape(rows * group, C_)
        assert torch.count_nonzero(dv[~slot_live.view(-1)]) == 0, "dlogits of a slot without loss is not exactly 0"
        full = d.as_strided((rows, d.stride(0)), (d.stride(0), 1))
        assert torch.count_nonzero(full[:, n_out:]) == 0
        res.append({"sum_count": sc, "lse": lse.view(rows, group)[slot_live].clone(), "dlogits": dv[slot_live.view(-1)].clone()})
    assert res[0]["dlogits"].abs().max() > 0
    _eq(res[0], res[1], f"fused head, group {group}")


# ---- pooling and broadcast -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [8, 31, 102])
def test_dense_pooling_ignores_masked_positions(gpu_device, dtype, S):
    valid = _valid_keys(S, arbitrary=S == 8)
    km = _key_mask(valid, S)
    dead = (~valid).reshape(-1).to(DEV)
    x = _rand(N_SEQ * S, 256, dtype=dtype, seed=S)
    xg = x.clone()
    xg[dead] = _garbage(N_SEQ * S, 256, dtype=dtype, seed=S + 1)[dead]
    dm = _rand(N_SEQ, 256, dtype=dtype, seed=S + 2)
    with _born_nan():
        dirty = ops.masked_mean_fwd(xg, km, N_SEQ, S)
        dx = ops.masked_mean_bwd(dm, km, N_SEQ, S)
    _eq([ops.masked_mean_fwd(x, km, N_SEQ, S), ops.masked_mean_bwd(dm, km, N_SEQ, S)], [dirty, dx], f"masked_mean S={S}")
    assert torch.count_nonzero(dx[dead]) == 0 and torch.count_nonzero(dx[~dead]) > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [30, 102])
def test_packed_pooling_ignores_the_bucket_rows(gpu_device, dtype, S):
    """packed rows behind seq_off[n_seq] up to total_rows: NaN in x, 0 in the gradient masked_mean_bwd returns"""
    lens = torch.tensor([1 + (11 * i) % S for i in range(N_SEQ)])
    lens[0], lens[1] = 1, S
    off = torch.zeros(N_SEQ + 1, dtype=torch.int32)
    off[1:] = lens.cumsum(0)
    real = int(off[-1])
    rows = (real + 127) // 128 * 128 + 64
    off = off.to(DEV)
    res = []
    for fill in (0.0, NAN):
        x = _rand(rows, 256, dtype=dtype, seed=S)
        x[real:] = fill
        with _born_nan(fill != fill):
            res.append([ops.masked_mean_fwd(x, None, N_SEQ, S, seq_off=off)])
    _eq(*res, f"packed masked_mean_fwd S={S}")
    dm = _rand(N_SEQ, 256, dtype=dtype, seed=S + 1)
    with _born_nan():
        dx = ops.masked_mean_bwd(dm, None, N_SEQ, S, seq_off=off, total_rows=rows)
    _eq([ops.masked_mean_bwd(dm, None, N_SEQ, S, seq_off=off, total_rows=rows)], [dx], f"packed masked_mean_bwd S={S}")
    assert dx.shape[0] == rows and torch.count_nonzero(dx[real:]) == 0 and bool(torch.isfinite(dx.float()).all())


def test_pack_tokens_ignores_what_follows_the_first_eos(gpu_device):
    """pack_tokens reads the tokens its key mask names: other commands and garbage arguments behind a sequence's end change
    nothing, and every row of its outputs is defined (rows past seq_off[-1] replicate token 0)"""
    from deepsvg_amd.synthetic import make_batch
    n, G, S = 3, 8, 32
    c, a = make_batch(n, G, S - 2, seed=3)
    cmd = c.view(n * G, S).contiguous().to(DEV)
    arg = a.view(n * G * S, -1).contiguous().float().to(DEV)
    km, _, _ = ops.build_masks(cmd, S, G, 4, want_group_mask=True)
    dead = ~((km.unsqueeze(1) >> torch.arange(S, device=DEV)) & 1).bool()
    dead[0, 0] = False                                          # token 0 is what the rows past the end replicate
    cg, ag = cmd.clone(), arg.clone()
    cg[dead] = 5.0                                              # another command id of the vocabulary
    ag[dead.view(-1)] = _garbage(n * G * S, arg.shape[1], dtype=torch.float32, seed=4)[dead.view(-1)]
    assert int(dead.sum()) > 0
    with _born_nan():
        dirty = ops.pack_tokens(cg.view(-1), ag, km, n * G, S)
    _eq(ops.pack_tokens(cmd.view(-1), arg, km, n * G, S), dirty, "pack_tokens")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_and_scatter_ignore_dead_rows(gpu_device, dtype):
    """gather_groups with n_src < n: rows of `src` behind its n_src groups are NaN, an index beyond them gives zeros.
    scatter_rows / live_rows: NaN in the source rows whose index is negative"""
    n, S, m = 9, 3, 5
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(DEV)
    res = []
    for fill in (0.0, NAN):
        src = _rand(n * S, 64, dtype=dtype, seed=2)
        src[m * S:] = fill
        with _born_nan(fill != fill):
            res.append([ops.gather_groups(src, perm, n, S, n_src=m)])
    _eq(*res, "gather_groups")
    zero_groups = (perm.long() >= m).repeat_interleave(S)
    assert torch.count_nonzero(res[1][0][zero_groups]) == 0 and torch.count_nonzero(res[1][0][~zero_groups]) > 0
    n_tok, group = 300, 6
    g = torch.Generator().manual_seed(4)
    w = (torch.rand(n_tok, group, generator=g) < 0.15).float()
    w[torch.rand(n_tok, generator=g) < 0.6] = 0.0
    live, count = ops.live_rows(w.view(-1).contiguous().to(DEV), group)
    n_live = int(count)
    rows = (n_live + 127) // 128 * 128
    idx = live[:rows].contiguous()
    assert 0 < n_live < rows and int(idx[n_live]) < 0
    for accumulate in (False, True):
        res = []
        for fill in (0.0, NAN):
            src = _rand(rows, 64, dtype=dtype, seed=5)
            src[n_live:] = fill
            with _born_nan(fill != fill):
                res.append([ops.scatter_rows(src, idx, torch.ones(n_tok, 64, device=DEV, dtype=dtype), accumulate=accumulate)])
        _eq(*res, f"scatter_rows accumulate={accumulate}")


# ---- accumulators handed over uninitialised (accumulate=False) -------------------------------------------------------------
def _accumulators(dtype, fill, defer):
    """layernorm_bwd's dgamma / dbeta, add_pos_bwd's d_pos, embed_scatter's three tables and bcast_add_bwd's column block of a
    wider buffer, all holding `fill` beforehand"""
    from deepsvg_amd.synthetic import make_batch
    f = lambda *s: torch.full(s, fill, device=DEV)
    rows, d = 1037, 256
    x, dy, res_ = (_rand(rows, d, dtype=dtype, seed=s) for s in (1, 2, 3))
    gamma = _rand(d, seed=4)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, gamma, 1e-5)
    n_seq, S = 33, 31
    dyp = _rand(n_seq * S, d, dtype=dtype, seed=5)
    c, a = make_batch(5, seed=4)
    T = c.numel()
    cmd, arg = c.view(-1).to(DEV), a.view(T, 11).float().to(DEV)
    groups = ops.group_index(c.view(-1, 32).contiguous().to(DEV), 32, 0).clamp(max=9)
    # small integers: the fp32 argument-table scatter adds with LDS float atomics inside a workgroup (csrc/embed.hip: the one
    # schedule-dependent sum of the package), and sums of small integers are exact in any order - so the comparison stays exact
    dA, dR = (_rand(T, 704, seed=6) * 2).round().to(dtype), (_rand(T, 256, seed=7) * 2).round().to(dtype)
    seed = _seed_tensor(42)
    out = {}

    def work():
        out["ln_dgamma"], out["ln_dbeta"] = f(d), f(d)
        out["ln_dx"] = ops.layernorm_bwd(dy, x, mean, rstd, gamma, res=res_, dgamma=out["ln_dgamma"], dbeta=out["ln_dbeta"])[0]
        out["lnm_dgamma"], out["lnm_dbeta"] = f(d), f(d)
        if dtype == torch.bfloat16:
            r = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dgamma=out["lnm_dgamma"], dbeta=out["lnm_dbeta"], masked=(0.1, 9, seed))
            out["lnm_dx"], out["lnm_dxm"] = r[0], r[3]
        else:
            ops.layernorm_bwd(dy, x, mean, rstd, gamma, dgamma=out["lnm_dgamma"], dbeta=out["lnm_dbeta"])
        out["d_pos"] = f(S, d)
        out["pos_dx"] = ops.add_pos_bwd(dyp, n_seq, S, out["d_pos"], drop_p=0.1, drop_site=5, seed=seed)
        out["d_arg"], out["d_cmd"], out["d_grp"] = f(257, 64), f(7, 256), f(10, 256)
        ops.embed_scatter(cmd, arg, dA, dR, out["d_arg"], out["d_cmd"], groups, out["d_grp"])
        out["bcast_dg"] = ops.bcast_add_bwd(dyp, n_seq, S, 0.1, 6, seed, n_seq_out=n_seq + 3)
    with _born_nan(fill != fill):
        if defer:
            with ops.DEFER:
                work()
            ops.flush_deferred()
        else:
            work()
    if dtype == torch.bfloat16:
        wide = torch.full((n_seq + 3, 1024), fill, device=DEV, dtype=dtype)
        ops.bcast_add_bwd(dyp, n_seq, S, 0.1, 6, seed, n_seq_out=n_seq + 3, out=wide[:, 512:768])
        torch.cuda.synchronize()
        assert _filled(wide[:, :512], fill) and _filled(wide[:, 768:], fill), "bcast_add_bwd wrote outside its column block"
        assert torch.equal(wide[:, 512:768], out["bcast_dg"])
    torch.cuda.synchronize()
    assert torch.count_nonzero(out["bcast_dg"][n_seq:]) == 0
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_accumulators_are_overwritten(gpu_device, dtype, defer):
    """accumulate=False means the accumulator's old contents are never read: pre-filled with NaN the results are finite and equal
    to those of zero-filled accumulators - immediately and for the deferred variants inside an `ops.DEFER` scope"""
    clean, dirty = _accumulators(dtype, 0.0, defer), _accumulators(dtype, NAN, defer)
    assert all(v.abs().max() > 0 for k, v in clean.items() if k.startswith(("d_", "ln"))), "a gradient is identically 0"
    _eq(clean, dirty, f"accumulators {dtype} defer={defer}")
