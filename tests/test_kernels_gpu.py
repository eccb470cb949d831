"""Every HIP kernel (through the C ABI / deepsvg_amd.ops) against its plain-PyTorch fp32 restatement
(tests/torch_ops_ref.py) on the same seeded inputs.  fp32 kernels: tight tolerances (exact-fp32 MFMA);
bf16 kernels: tolerances of bf16 storage rounding, stated per test."""
import numpy as np
import pytest
import torch

from deepsvg_amd import lib, ops
from tests import torch_ops_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


def _tol(dtype, k=1):
    """relative-to-max tolerance: fp32 accumulate error grows ~sqrt(k); bf16 adds 2^-8 storage rounding"""
    return 2e-6 * max(1.0, k ** 0.5) if dtype == torch.float32 else 1.2e-2


def _close(a, b, tol, what=""):
    a, b = a.float(), b.float()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol:.1e})"


def _rand(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def _seed_tensor(v=0x1234567887654321):
    return torch.tensor([v if v < (1 << 63) else v - (1 << 64)], dtype=torch.int64, device=DEV)


# ----------------------------------------------------------------------------------------------------
def test_library_loads_and_reports_version(gpu_device):
    from deepsvg_amd import lib
    assert lib.load().dsvg_version() >= 1


def test_trread_probe_semantics(gpu_device):
    """ds_read_b64_tr_b16: within each 16-lane group, lane i / element j receives the element that lane
    (4*j + i//4) of the group loaded at position (i % 4).  With per-lane addresses l*8 bytes (a contiguous
    4x16 row-major b16 matrix per group) lane i therefore gets column i: img[g*64 + j*16 + i]."""
    off = (torch.arange(64, dtype=torch.int32) * 8).to(DEV)
    out = ops.probe_trread(off).cpu().view(64, 4)
    exp = torch.empty(64, 4, dtype=torch.int16)
    for l in range(64):
        g, i = l // 16, l % 16
        for j in range(4):
            exp[l, j] = g * 64 + j * 16 + i
    print("trread probe lanes 0..19:\n", out[:20].tolist())
    assert torch.equal(out, exp), "ds_read_b64_tr_b16 semantics differ from the assumed 4x16 transpose"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(300, 200, 64), (257, 768, 256), (128, 7, 512), (520, 264, 1000)])
def test_gemm_layouts(gpu_device, dtype, impl, a_kc, b_kc, M, N, K):
    pad = 8
    Mp, Np, Kp = (M + pad - 1) // pad * pad, (N + pad - 1) // pad * pad, (K + pad - 1) // pad * pad
    # operands live in padded buffers (row stride multiple of 8) like the model's internal buffers
    a_full = _rand(M if a_kc else K, Kp if a_kc else Mp, dtype=dtype, seed=1)
    b_full = _rand(N if b_kc else K, Kp if b_kc else Np, dtype=dtype, seed=2)
    a = a_full[:, :K] if a_kc else a_full[:, :M]
    b = b_full[:, :K] if b_kc else b_full[:, :N]
    bias = _rand(N, seed=3)
    out = ops.gemm(a, b, a_kc=a_kc, b_kc=b_kc, bias=bias, impl=impl)
    ref = R.gemm(a, b, a_kc=a_kc, b_kc=b_kc, bias=bias, out_dtype=torch.float32)
    _close(out, ref, _tol(dtype, K), f"gemm {M}x{N}x{K} akc={a_kc} bkc={b_kc} impl={impl}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_asymmetric_identity(gpu_device, dtype):
    """A = I with an asymmetric B catches a transposed C write (guide rule G9)"""
    n = 160
    a = torch.eye(n, device=DEV, dtype=dtype)
    b = (torch.arange(n * n, device=DEV, dtype=torch.float32).view(n, n) % 251 / 16.0).to(dtype)
    out = ops.gemm(a, b, b_kc=False)          # C = I @ B
    assert torch.equal(out.float(), b.float())
    out2 = ops.gemm(a, b, b_kc=True)          # C = I @ B^T
    assert torch.equal(out2.float(), b.float().t())


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogues(gpu_device, dtype):
    M, N, K = 384, 512, 256
    a, b = _rand(M, K, dtype=dtype, seed=4), _rand(N, K, dtype=dtype, seed=5, scale=0.1)
    bias, res = _rand(N, seed=6), _rand(M, N, dtype=dtype, seed=7)
    gate = _rand(M, N, dtype=dtype, seed=8)
    seed = _seed_tensor()
    tol = _tol(dtype, K)
    for kw in [dict(bias=bias, act=R.RELU), dict(bias=bias, res=res), dict(bias=bias, res=res, res_pre=True, act=R.RELU),
               dict(gate=gate, gate_scale=1.25), dict(bias=bias, res=res, drop_p=0.1, drop_site=7, seed=seed),
               # the embedding's epilogue: residual INSIDE the dropout (a run-time switch of the LDS-DMA kernel's epilogue)
               dict(bias=bias, res=res, res_pre=True, drop_p=0.1, drop_site=7, seed=seed), dict(bias=bias, res=res, res_pre=True),
               dict(bias=bias, act=R.RELU, drop_p=0.3, drop_site=9, seed=seed),
               dict(a_drop_p=0.1, a_drop_site=11, seed=seed)]:
        out = ops.gemm(a, b, **kw)
        ref = R.gemm(a, b, out_dtype=torch.float32, **kw)
        _close(out, ref, tol, f"epilogue {sorted(kw)}")
    # in-place residual (C aliases res) and accumulate
    x = res.clone()
    ops.gemm(a, b, bias=bias, res=x, out=x)
    _close(x, R.gemm(a, b, bias=bias, res=res, out_dtype=torch.float32), tol, "in-place residual")
    acc = torch.ones(M, N, device=DEV, dtype=torch.float32)
    ops.gemm(a, b, out=acc, accumulate=True)
    _close(acc, 1.0 + R.gemm(a, b, out_dtype=torch.float32), tol, "accumulate")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_weight_grad_splitk_with_dropout_replay(gpu_device, dtype):
    """dW[n,k] = sum_t drop(dy)[t,n] x[t,k]: TN layout, split over tokens, dropout mask replayed on dy"""
    T, n_out, k_in = 4100, 512, 256
    dy, x = _rand(T, n_out, dtype=dtype, seed=9), _rand(T, k_in, dtype=dtype, seed=10)
    seed = _seed_tensor(0xDEADBEEFCAFEF00D)
    out = torch.empty(n_out, k_in, device=DEV, dtype=torch.float32)
    ops.gemm(dy, x, a_kc=False, b_kc=False, out=out, a_drop_p=0.1, a_drop_site=3, seed=seed,
             split_k=ops.split_k_for(n_out, k_in, T))
    ref = R.gemm(dy, x, a_kc=False, b_kc=False, a_drop_p=0.1, a_drop_site=3, seed=seed, out_dtype=torch.float32)
    _close(out, ref, _tol(dtype, T), "dW split-k")
    bs = ops.colsum(dy, drop_p=0.1, drop_site=3, seed=seed)
    _close(bs, R.colsum(dy, drop_p=0.1, drop_site=3, seed=seed), _tol(dtype, T), "colsum")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_out,k_in,split", [(4100, 512, 256, 16), (992, 2827, 256, 4), (3000, 7, 256, 8), (640, 256, 704, 3)])
def test_gemm_weight_grad_with_fused_bias_rowsum(gpu_device, dtype, T, n_out, k_in, split):
    """dW and db from ONE split-K GEMM: rowsum[m] = sum_t dy[t, m] via an MFMA against ones"""
    ld = (n_out + 7) // 8 * 8
    buf = torch.zeros(T, ld, device=DEV, dtype=dtype)
    buf[:, :n_out] = _rand(T, n_out, dtype=dtype, seed=21)
    dy, x = buf[:, :n_out], _rand(T, k_in, dtype=dtype, seed=22)
    dw = torch.empty(n_out, k_in, device=DEV, dtype=torch.float32)
    db = torch.empty(n_out, device=DEV, dtype=torch.float32)
    ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=split, rowsum=db)
    _close(dw, R.gemm(dy, x, a_kc=False, b_kc=False, out_dtype=torch.float32), _tol(dtype, T), "dW")
    _close(db, dy.float().sum(0), 1e-5 * T ** 0.5 if dtype == torch.float32 else 1e-2, "fused bias grad")


@pytest.mark.parametrize("stages", [4, 3, 6])
@pytest.mark.parametrize("M,N,K", [(384, 512, 256), (1000, 264, 512), (129, 8, 64), (4096, 768, 256)])
def test_gemm_lds_dma_kernel_equals_register_staged_kernel(gpu_device, stages, M, N, K):
    """The LDS-DMA bf16 kernel (impl 3/4: swizzled DMA images, swapped MFMA, register epilogue) must reproduce the
    register-staged kernel (impl 2) BIT FOR BIT on every epilogue it implements: same k order, same epilogue order."""
    dtype = torch.bfloat16
    a, w = _rand(M, K, dtype=dtype, seed=31), _rand(N, K, dtype=dtype, seed=32, scale=0.1)
    wt = _rand(K, N, dtype=dtype, seed=33, scale=0.1)          # [k][n] weight view for the input-gradient layout
    bias, res, gate = _rand(N, seed=34), _rand(M, N, dtype=dtype, seed=35), _rand(M, N, dtype=dtype, seed=36)
    seed = _seed_tensor(0x0123456789ABCDEF)
    cases = [(w, dict(bias=bias)), (w, dict()), (w, dict(bias=bias, res=res, drop_p=0.1, drop_site=5, seed=seed)),
             (w, dict(bias=bias, res=res)), (w, dict(bias=bias, act=R.RELU, drop_p=0.2, drop_site=6, seed=seed)),
             (wt, dict(b_kc=False)), (wt, dict(b_kc=False, gate=gate, gate_scale=1.0 / 0.9))]
    for b, kw in cases:
        new = ops.gemm(a, b, impl=stages, **kw)
        old = ops.gemm(a, b, impl=2, **kw)
        assert torch.equal(new, old), f"LDS-DMA kernel differs from the register-staged kernel: {sorted(kw)} {M}x{N}x{K}"
        _close(new, R.gemm(a, b, out_dtype=torch.float32, **kw), _tol(dtype, K), f"glds {sorted(kw)}")


@pytest.mark.parametrize("stages", [4, 3, 6])
def test_gemm_lds_dma_ragged_head_shapes(gpu_device, stages):
    """N = 523 (like the 2827-wide argument head: not a multiple of 8) in a row-padded buffer: forward through the
    LDS-DMA kernel (last 8-column chunk finished element-wise), bit-identical to the register-staged kernel, and the
    weight gradient with a ragged M (the LDS-DMA kernel keeps its split-K slices in bf16, the register-staged one in
    fp32, so those two agree to the slices' rounding, not bit for bit)"""
    dtype = torch.bfloat16
    T, N, K, ld = 1920, 523, 256, 528
    x, w, bias = _rand(T, K, dtype=dtype, seed=81), _rand(N, K, dtype=dtype, seed=82, scale=0.1), _rand(N, seed=83)
    outs = []
    for impl in (stages, 2):
        buf = torch.full((T, ld), 7.0, device=DEV, dtype=dtype)
        ops.gemm(x, w, bias=bias, out=buf[:, :N], impl=impl)
        assert torch.all(buf[:, N:] == 7.0), "wrote into the row padding"
        outs.append(buf[:, :N].clone())
    assert torch.equal(outs[0], outs[1])
    _close(outs[0], R.gemm(x, w, bias=bias, out_dtype=torch.float32), _tol(dtype, K), "ragged-N forward")
    # round 6: a bias that starts on a 4-byte, not a 16-byte, boundary (a row range of a longer vector: the argument head's slots in
    # use, functional.ArgsHeadLossFn) goes through the LDS-DMA kernel as well - same numbers, no copy of the bias
    for off in (1, 2, 3):
        longer = torch.zeros(N + 8, device=DEV)
        longer[off:off + N] = bias
        buf = torch.full((T, ld), 7.0, device=DEV, dtype=dtype)
        assert longer[off:off + N].data_ptr() % 16 == 4 * off
        ops.gemm(x, w, bias=longer[off:off + N], out=buf[:, :N], impl=stages)
        assert torch.equal(buf[:, :N], outs[0]) and torch.all(buf[:, N:] == 7.0), off
    dbuf = torch.zeros(T, ld, device=DEV, dtype=dtype)
    dbuf[:, :N] = _rand(T, N, dtype=dtype, seed=84)
    dy = dbuf[:, :N]
    res = []
    for impl in (stages, 2):
        flat = torch.empty(N * K + N, device=DEV, dtype=torch.float32)
        dw, db = flat[:N * K].view(N, K), flat[N * K:]
        ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=8, rowsum=db, impl=impl)
        res.append((dw.clone(), db.clone()))
    _close(res[0][0], res[1][0], 4e-3, "ragged-M dW: bf16 split-K slices vs fp32 slices")
    _close(res[0][0], R.gemm(dy, x, a_kc=False, b_kc=False, out_dtype=torch.float32), _tol(dtype, T), "ragged-M dW")
    _close(res[0][1], dy.float().sum(0), 1e-2, "ragged-M bias grad")


@pytest.mark.parametrize("stages", [4, 3, 6])
@pytest.mark.parametrize("T,n_out,k_in,split", [(4096, 512, 256, 16), (1920, 256, 512, 8), (640, 264, 704, 3),
                                                (8192, 768, 256, 64)])
def test_gemm_lds_dma_weight_grad(gpu_device, stages, T, n_out, k_in, split):
    """split-K weight gradient + fused bias row sums through the LDS-DMA kernel (both operands token-major, hardware
    transpose reads from the swizzled image): partial sums identical to the register-staged kernel"""
    dtype = torch.bfloat16
    dy, x = _rand(T, n_out, dtype=dtype, seed=41), _rand(T, k_in, dtype=dtype, seed=42)
    outs = {}
    for impl in (stages, 2):
        dw = torch.empty(n_out, k_in, device=DEV, dtype=torch.float32)
        db = torch.empty(n_out, device=DEV, dtype=torch.float32)
        ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=split, rowsum=db, impl=impl)
        dw2 = torch.empty(n_out, k_in, device=DEV, dtype=torch.float32)
        ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw2, split_k=split, impl=impl)
        assert torch.equal(dw, dw2)
        outs[impl] = (dw, db)
    _close(outs[stages][0], outs[2][0], 4e-3, "dW: bf16 split-K slices (LDS-DMA kernel) vs fp32 slices (register-staged)")
    _close(outs[stages][0], R.gemm(dy, x, a_kc=False, b_kc=False, out_dtype=torch.float32), _tol(dtype, T), "dW")
    _close(outs[stages][1], dy.float().sum(0), 1e-2, "fused bias grad (v_dot2c row sums)")
    _close(outs[stages][1], outs[2][1], 1e-5, "row sums: dot2 vs MFMA-against-ones")


def test_deferred_zero_fills_ride_on_the_flush(gpu_device):
    """ops.zero_ (dsvg_defer_zero, round 5): inside an open deferral scope a fill is queued as a reduction over zero partial rows -
    the tensor keeps its old contents until flush_deferred() and is zero afterwards, whatever its width and alignment (16-byte
    multiples, odd widths, a single element); a reduction into an overlapping destination afterwards still wins; outside a scope
    it is a plain fill."""
    base = torch.full((3 * 4096 + 64,), 7.0, device=DEV, dtype=torch.float32)
    views = [base[0:4096], base[4096 + 1:4096 + 1 + 2827], base[2 * 4096 + 3:2 * 4096 + 4], base[3 * 4096:3 * 4096 + 8]]
    dy, x = _rand(512, 64, dtype=torch.bfloat16, seed=1), _rand(512, 32, dtype=torch.bfloat16, seed=2)
    want = torch.empty(64, 32, device=DEV, dtype=torch.float32)
    ops.gemm(dy, x, a_kc=False, b_kc=False, out=want, split_k=4)
    over = torch.full((64 * 32,), 3.0, device=DEV, dtype=torch.float32)
    with ops.DEFER:
        for v in views:
            assert ops.zero_(v) is v
        torch.cuda.synchronize()
        assert all(bool((v == 7.0).all()) for v in views), "a queued fill must not run before the flush"
        ops.zero_(over)
        ops.gemm(dy, x, a_kc=False, b_kc=False, out=over.view(64, 32), split_k=4)       # overlapping destination: the queue runs first
    ops.flush_deferred()
    torch.cuda.synchronize()
    assert all(bool((v == 0).all()) for v in views)
    touched = torch.zeros_like(base, dtype=torch.bool)
    for lo, n in ((0, 4096), (4097, 2827), (2 * 4096 + 3, 1), (3 * 4096, 8)):
        touched[lo:lo + n] = True
    assert bool((base[~touched] == 7.0).all()), "a fill wrote outside its tensor"
    _close(over.view(64, 32), want, 2e-6, "reduction into a destination with a queued fill")
    t = torch.ones(100, device=DEV)
    ops.zero_(t[1:])
    assert float(t.sum()) == 1.0 and not ops._DEFER.state


def test_deferred_reductions_match_immediate_ones(gpu_device):
    """ops.DEFER queues the partial-sum reductions (bf16 / fp32 split-K slices with and without fused row sums, ragged M,
    LayerNorm gamma/beta partials, bias column sums); flush_deferred() performs them, 64 per launch (a 150-entry queue =
    3 launches), in a fixed summation order that differs from the immediate kernels' - hence the 2e-6 tolerance.  A
    second reduction into a queued destination flushes the queue first, so accumulate=True keeps its meaning."""
    def work():
        outs = []
        for i, (T, n_out, k_in, split, dtype) in enumerate([(4096, 512, 256, 16, torch.bfloat16), (1920, 256, 512, 8, torch.bfloat16),
                                                           (640, 264, 704, 3, torch.bfloat16), (8192, 768, 256, 64, torch.bfloat16),
                                                           (1920, 523, 256, 8, torch.bfloat16), (4100, 512, 256, 16, torch.float32),
                                                           (992, 2827, 256, 4, torch.bfloat16)]):
            ld = (n_out + 7) // 8 * 8
            buf = torch.zeros(T, ld, device=DEV, dtype=dtype)
            buf[:, :n_out] = _rand(T, n_out, dtype=dtype, seed=300 + i)
            dy, x = buf[:, :n_out], _rand(T, k_in, dtype=dtype, seed=400 + i)
            flat = torch.empty(n_out * k_in + n_out, device=DEV, dtype=torch.float32)
            dw, db = flat[:n_out * k_in].view(n_out, k_in), flat[n_out * k_in:]
            ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=split, rowsum=db)       # dW | db adjacent: one segment
            dw2 = torch.empty(n_out, k_in, device=DEV, dtype=torch.float32)
            db2 = torch.empty(n_out, device=DEV, dtype=torch.float32)
            ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw2, split_k=split, rowsum=db2)     # two segments
            outs += [flat, dw2, db2, ops.colsum(dy)]
        for j, (rows, d) in enumerate([(4133, 256), (96, 256), (20000, 512)]):
            xx, dyy = _rand(rows, d, dtype=torch.bfloat16, seed=500 + j), _rand(rows, d, dtype=torch.bfloat16, seed=510 + j)
            g = _rand(d, seed=520 + j)
            _, mean, rstd = ops.layernorm_fwd(xx, g, g, 1e-5)
            outs += list(ops.layernorm_bwd(dyy, xx, mean, rstd, g))
        # the same small reduction 150 times into distinct outputs, then twice more into ONE output with accumulate
        dy, x = _rand(512, 64, dtype=torch.bfloat16, seed=600), _rand(512, 32, dtype=torch.bfloat16, seed=601)
        many = torch.zeros(150, 64, 32, device=DEV, dtype=torch.float32)
        for i in range(150):
            ops.gemm(dy, x, a_kc=False, b_kc=False, out=many[i], split_k=4)
        acc = torch.ones(64, 32, device=DEV, dtype=torch.float32)
        for _ in range(3):
            ops.gemm(dy, x, a_kc=False, b_kc=False, out=acc, split_k=4, accumulate=True)
        return outs + [many, acc]

    want = work()
    L = __import__("deepsvg_amd.lib", fromlist=["load"]).load()
    sk = torch.cuda.current_stream().cuda_stream
    other = torch.cuda.Stream()
    with ops.DEFER:
        got = work()
        assert L.dsvg_defer_scope(1, sk) > 0, "nothing was queued"
        # the queue belongs to the stream: the same launches on another stream are neither queued nor flushed by it
        other.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            elsewhere = work()
            assert L.dsvg_defer_scope(0, other.cuda_stream) == 0, "a launch on another stream was queued"
        torch.cuda.current_stream().wait_stream(other)
        assert L.dsvg_defer_scope(1, sk) > 0
    ops.flush_deferred()
    assert L.dsvg_defer_scope(0, sk) == 0 and not ops._DEFER.state
    torch.cuda.synchronize()
    for a, b in zip(elsewhere, want):
        assert torch.equal(a, b), "launches on a stream without an open scope must reduce immediately"
    for i, (a, b) in enumerate(zip(got, want)):
        _close(a, b, 2e-6, f"deferred reduction output {i}")
    assert torch.equal(got[-2][0], got[-2][149])
    again = work()          # outside the scope nothing is queued
    assert L.dsvg_defer_scope(0, sk) == 0
    for a, b in zip(again, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_args_head_shapes(gpu_device, dtype):
    """N = 11*257 = 2827 (not a multiple of 8): forward, dX with a padded-stride dlogits, dW"""
    T, d, N = 992, 256, 2827
    x, w = _rand(T, d, dtype=dtype, seed=11), _rand(N, d, dtype=dtype, seed=12, scale=0.05)
    bias = _rand(N, seed=13)
    y = ops.gemm(x, w, bias=bias)
    _close(y, R.gemm(x, w, bias=bias, out_dtype=torch.float32), _tol(dtype, d), "args head fwd")
    ld = 2832
    dbuf = torch.zeros(T, ld, device=DEV, dtype=dtype)
    dbuf[:, :N] = _rand(T, N, dtype=dtype, seed=14)
    dy = dbuf[:, :N]
    dx = ops.gemm(dy, w, b_kc=False)
    _close(dx, R.gemm(dy, w, b_kc=False, out_dtype=torch.float32), _tol(dtype, N), "args head dX")
    dw = torch.empty(N, d, device=DEV, dtype=torch.float32)
    ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=4)
    _close(dw, R.gemm(dy, x, a_kc=False, b_kc=False, out_dtype=torch.float32), _tol(dtype, T), "args head dW")


# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", [(1000, 256), (37, 512), (5000, 64)])
def test_layernorm(gpu_device, dtype, rows, d):
    x = _rand(rows, d, dtype=dtype, seed=1) * 2 + 0.5
    gamma, beta = _rand(d, seed=2) * 0.1 + 1, _rand(d, seed=3) * 0.1
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    yr, mr, rr = R.layernorm_fwd(x, gamma, beta)
    tol = 5e-6 if dtype == torch.float32 else 1e-2
    _close(y, yr, tol, "ln fwd")
    _close(mean, mr, 1e-5, "ln mean")
    _close(rstd, rr, 1e-5, "ln rstd")
    dy, res = _rand(rows, d, dtype=dtype, seed=4), _rand(rows, d, dtype=dtype, seed=5)
    dx, dg, db = ops.layernorm_bwd(dy, x, mean, rstd, gamma, res=res)
    dxr, dgr, dbr = R.layernorm_bwd(dy, x, mean, rstd, gamma, res=res)
    _close(dx, dxr, tol, "ln dx")
    _close(dg, dgr, 2e-5 if dtype == torch.float32 else 1e-2, "ln dgamma")
    _close(db, dbr, 2e-5 if dtype == torch.float32 else 1e-2, "ln dbeta")
    # in-place residual (dx aliases res)
    r2 = res.clone()
    ops.layernorm_bwd(dy, x, mean, rstd, gamma, res=r2, dx=r2)
    _close(r2, dxr, tol, "ln dx in place")
    # second output (round 5): dx with a dropout mask replayed on it - bit-identical to drop_apply on the stored dx, the
    # other three results bit-identical to the plain launch
    seed = _seed_tensor(0x77AA55)
    for p_ in (0.1, 0.0):
        dx2, dg2, db2, dxm = ops.layernorm_bwd(dy, x, mean, rstd, gamma, res=res, masked=(p_, 417, seed))
        assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)
        assert torch.equal(dxm, ops.drop_apply(dx, p_, 417, seed) if p_ > 0 else dx)


def _key_masks(n_seq, S, seed, all_valid=False):
    if all_valid:
        return None
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, S + 1, (n_seq,), generator=g)
    return ((1 << lens.to(torch.int64)) - 1).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,n_seq,masked", [(32, 40, True), (31, 33, False), (8, 100, True), (8, 64, False),
                                             (52, 6, True), (16, 9, True), (5, 7, False)])
def test_attention(gpu_device, dtype, S, n_seq, masked):
    H = 8
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=S)
    km = _key_masks(n_seq, S, seed=S + 1, all_valid=not masked)
    if masked and S == 8:   # arbitrary (non-prefix) visibility patterns, at least one visible key
        g = torch.Generator().manual_seed(99)
        km = (torch.randint(1, 256, (n_seq,), generator=g)).to(torch.int64).to(DEV)
    scale = 32 ** -0.5
    seed = _seed_tensor(0x0123456789ABCDEF)
    tol = 3e-6 if dtype == torch.float32 else 1.5e-2
    for p in (0.0, 0.1):
        o = ops.attention_fwd(qkv, km, n_seq, S, H, scale, p, 21, seed)
        orf = R.attention_fwd(qkv.float(), km, n_seq, S, H, scale, p, 21, seed)
        _close(o, orf, tol, f"attn fwd S={S} p={p}")
        do = _rand(n_seq * S, 32 * H, dtype=dtype, seed=S + 2)
        dq = ops.attention_bwd(qkv, km, do, n_seq, S, H, scale, p, 21, seed)
        dqr = R.attention_bwd(qkv.float(), km, do.float(), n_seq, S, H, scale, p, 21, seed)
        _close(dq, dqr, 1e-5 if dtype == torch.float32 else 2e-2, f"attn bwd S={S} p={p}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,n_seq,masked", [(8, 9, False), (31, 20, True), (32, 7, True), (51, 13, True), (64, 5, False), (60, 5, True),
                                            (1, 4, False), (17, 6, False)])
def test_attention_causal(gpu_device, dtype, S, n_seq, masked):
    """autoregressive decoder: query i attends keys j <= i (and only those the key-padding mask allows)"""
    H = 8
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=S + 40)
    km = _key_masks(n_seq, S, seed=S + 41, all_valid=not masked)        # valid prefixes: key 0 is always visible
    scale = 32 ** -0.5
    seed = _seed_tensor(0x0FEDCBA987654321)
    for p in (0.0, 0.1):
        o = ops.attention_fwd(qkv, km, n_seq, S, H, scale, p, 23, seed, causal=True)
        orf = R.attention_fwd(qkv.float(), km, n_seq, S, H, scale, p, 23, seed, causal=True)
        _close(o, orf, 3e-6 if dtype == torch.float32 else 1.5e-2, f"causal attn fwd S={S} p={p}")
        do = _rand(n_seq * S, 32 * H, dtype=dtype, seed=S + 42)
        dq = ops.attention_bwd(qkv, km, do, n_seq, S, H, scale, p, 23, seed, causal=True)
        dqr = R.attention_bwd(qkv.float(), km, do.float(), n_seq, S, H, scale, p, 23, seed, causal=True)
        _close(dq, dqr, 1e-5 if dtype == torch.float32 else 2e-2, f"causal attn bwd S={S} p={p}")
    if S > 1:       # the first query row depends on key 0 alone: its output is v_0
        v0 = qkv.float().view(n_seq, S, 3, H * 32)[:, 0, 2]
        o0 = ops.attention_fwd(qkv, km, n_seq, S, H, scale, causal=True).float().view(n_seq, S, H * 32)[:, 0]
        _close(o0, v0, 1e-6 if dtype == torch.float32 else 1e-2, "first causal row")


# ----------------------------------------------------------------------------------------------------
def _packed_case(n_seq, S, seed):
    """random valid-prefix lengths in 1..S -> (key_mask int64 [n_seq], seq_off int32 [n_seq+1], total)"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, S + 1, (n_seq,), generator=g)
    lens[0], lens[-1] = S, 1
    km = ((torch.ones_like(lens) << lens) - 1).to(torch.int64).to(DEV)
    off = torch.zeros(n_seq + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).to(torch.int32)
    return km, off.to(DEV), int(off[-1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,n_seq", [(32, 70), (31, 40), (8, 50)])
def test_attention_packed_layout(gpu_device, dtype, S, n_seq):
    """variable-length sequences packed back to back (first encoder stage): forward and backward against the padded
    reference, pad rows zero-filled; S = 32 / 31 bf16 runs the MFMA kernel, the rest the VALU kernel"""
    H_, d = 8, 256
    km, off, total = _packed_case(n_seq, S, 5)
    rows = (total + 127) // 128 * 128
    qkv = _rand(rows, 3 * d, dtype=dtype, seed=50)
    do = _rand(rows, d, dtype=dtype, seed=51)
    seed = _seed_tensor(0x1111222233334444)
    for p in (0.0, 0.2):
        out = ops.attention_fwd(qkv, None, n_seq, S, H_, 32 ** -0.5, p, 17, seed, seq_off=off)
        ref = R.attention_fwd(qkv, None, n_seq, S, H_, 32 ** -0.5, p, 17, seed, seq_off=off)
        _close(out, ref, 2e-5 if dtype == torch.float32 else 2e-2, f"packed attention fwd p={p}")
        assert torch.count_nonzero(out[total:]) == 0
        dq = ops.attention_bwd(qkv, None, do, n_seq, S, H_, 32 ** -0.5, p, 17, seed, seq_off=off)
        dref = R.attention_bwd(qkv, None, do, n_seq, S, H_, 32 ** -0.5, p, 17, seed, seq_off=off)
        _close(dq, dref, 5e-5 if dtype == torch.float32 else 3e-2, f"packed attention bwd p={p}")
        assert torch.count_nonzero(dq[total:]) == 0
        # several short sequences per workgroup (block-diagonal 32-row tiles): same numbers
        tiles = ops.attention_tiles(off, n_seq, 32)
        ref_t = R.attention_tiles(off, n_seq, 32)
        n_tiles = int(ref_t[n_seq + 1])
        assert int(tiles[n_seq + 1]) == n_tiles and torch.equal(tiles[:n_tiles + 1], ref_t[:n_tiles + 1])
        out_t = ops.attention_fwd(qkv, None, n_seq, S, H_, 32 ** -0.5, p, 17, seed, seq_off=off, tiles=tiles)
        dq_t = ops.attention_bwd(qkv, None, do, n_seq, S, H_, 32 ** -0.5, p, 17, seed, seq_off=off, tiles=tiles)
        _close(out_t, ref, 2e-5 if dtype == torch.float32 else 2e-2, f"tiled packed attention fwd p={p}")
        _close(dq_t, dref, 5e-5 if dtype == torch.float32 else 3e-2, f"tiled packed attention bwd p={p}")
        assert torch.count_nonzero(out_t[total:]) == 0 and torch.count_nonzero(dq_t[total:]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_over_a_sequence_prefix(gpu_device, dtype):
    """dense layout, n_seq sequences followed by rows that must come back as zeros (visible-first decoder order)"""
    H_, d, S, n_seq, rows = 8, 256, 31, 37, 1280
    qkv, do = _rand(rows, 3 * d, dtype=dtype, seed=70), _rand(rows, d, dtype=dtype, seed=71)
    dq = ops.attention_bwd(qkv, None, do, n_seq, S, H_, 32 ** -0.5)
    ref = R.attention_bwd(qkv, None, do, n_seq, S, H_, 32 ** -0.5)
    _close(dq, ref, 5e-5 if dtype == torch.float32 else 3e-2, "prefix attention bwd")
    assert torch.count_nonzero(dq[n_seq * S:]) == 0
    out = ops.attention_fwd(qkv, None, n_seq, S, H_, 32 ** -0.5)
    _close(out, R.attention_fwd(qkv, None, n_seq, S, H_, 32 ** -0.5), 2e-5 if dtype == torch.float32 else 2e-2, "fwd")
    assert torch.count_nonzero(out[n_seq * S:]) == 0


def test_visible_first_and_gather_groups(gpu_device):
    g = torch.Generator().manual_seed(9)
    for n in (5, 1024, 4099):
        vis = (torch.rand(n, generator=g) < 0.56).to(torch.int32).to(DEV)
        got = ops.visible_first(vis)
        exp = R.visible_first(vis)
        for a, b, what in zip(got, exp, ("new_of_old", "old_of_new", "n_visible")):
            assert torch.equal(a, b), f"visible_first {what} n={n}"
        for dtype in DTYPES:
            x = _rand(n * 3, 64, dtype=dtype, seed=n)
            y = ops.gather_groups(x, got[1], n, 3)
            assert torch.equal(y, R.gather_groups(x, got[1], n, 3))
            assert torch.equal(ops.gather_groups(y, got[0], n, 3), x)       # the inverse permutation restores x
            # a source that holds the leading groups only: the others come out as zero sequences; and the leading
            # groups of the permutation only (the two halves of a stage that ran on a prefix of its sequences)
            m = (n + 1) // 2
            part = ops.gather_groups(x, got[1], m, 3)
            assert torch.equal(part, y[:m * 3])
            back = ops.gather_groups(part, got[0], n, 3, n_src=m)
            assert torch.equal(back, R.gather_groups(part, got[0], n, 3, n_src=m))
            keep = (got[0].long() < m).repeat_interleave(3).unsqueeze(1).to(x.dtype)
            assert torch.equal(back, x * keep)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_tokens_and_packed_mean(gpu_device, dtype):
    n, G, S = 6, 8, 32
    cmd, arg = _cmd_args(n, G, S - 2, seed=3)
    cmd2 = cmd.view(n * G, S).contiguous()
    arg2 = arg.view(n * G * S, -1).contiguous()
    km, _, _ = ops.build_masks(cmd2, S, G, 4, want_group_mask=True)
    got = ops.pack_tokens(cmd2.view(-1), arg2, km, n * G, S)
    exp = R.pack_tokens(cmd2.view(-1), arg2, km, n * G, S)
    for a, b, what in zip(got, exp, ("seq_off", "commands", "args", "pos")):
        assert torch.equal(a, b), f"pack_tokens {what}"
    off = got[0]
    total = int(off[-1])
    rows = (total + 127) // 128 * 128
    x = _rand(rows, 256, dtype=dtype, seed=60)
    m = ops.masked_mean_fwd(x, None, n * G, S, seq_off=off)
    _close(m, R.masked_mean_fwd(x, None, n * G, S, seq_off=off), 1e-6 if dtype == torch.float32 else 1e-2, "packed mean")
    dm = _rand(n * G, 256, dtype=dtype, seed=61)
    dx = ops.masked_mean_bwd(dm, None, n * G, S, seq_off=off, total_rows=rows)
    _close(dx, R.masked_mean_bwd(dm, None, n * G, S, seq_off=off, total_rows=rows),
           1e-6 if dtype == torch.float32 else 1e-2, "packed mean bwd")
    assert torch.count_nonzero(dx[total:]) == 0


def _cmd_args(n, G=8, S=30, seed=0):
    from deepsvg_amd.synthetic import make_batch
    c, a = make_batch(n, G, S, seed=seed)
    return c.to(DEV), a.to(DEV)


def test_masks_and_group_index(gpu_device):
    c, _ = _cmd_args(37, seed=3)
    cmd = c.view(-1, 32).contiguous()
    km, vis, gm = ops.build_masks(cmd, 32, 8, 4, want_group_mask=True)
    kmr, visr, gmr = R.build_masks(cmd, 32, 8, 4, want_group_mask=True)
    assert torch.equal(km, kmr) and torch.equal(vis, visr) and torch.equal(gm, gmr)
    gi = ops.group_index(cmd, 32, 0)
    assert torch.equal(gi, R.group_index(cmd, 32, 0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_embedding_gather_scatter(gpu_device, dtype):
    c, a = _cmd_args(21, seed=4)
    T = c.numel()
    cmd, arg = c.view(-1), a.view(T, 11)
    ce, ae, ge = _rand(7, 256, seed=1), _rand(257, 64, seed=2), _rand(10, 256, seed=3)
    groups = ops.group_index(c.view(-1, 32).contiguous(), 32, 0).clamp(max=9)
    A, Rr = ops.embed_gather(cmd, arg, ce, ae, dtype, ge, groups)
    Ar, Rrr = R.embed_gather(cmd, arg, ce, ae, torch.float32, ge, groups)
    tol = 0.0 if dtype == torch.float32 else 8e-3
    _close(A, Ar, tol + 1e-12, "gather A")
    _close(Rr, Rrr, tol + 1e-7, "gather R")
    dA, dR = _rand(T, 704, dtype=dtype, seed=5), _rand(T, 256, dtype=dtype, seed=6)
    d_arg, d_cmd, d_grp = (torch.empty(257, 64, device=DEV), torch.empty(7, 256, device=DEV),
                           torch.empty(10, 256, device=DEV))
    ops.embed_scatter(cmd, arg, dA, dR, d_arg, d_cmd, groups, d_grp)
    r_arg, r_cmd, r_grp = torch.empty_like(d_arg), torch.empty_like(d_cmd), torch.empty_like(d_grp)
    R.embed_scatter(cmd, arg, dA, dR, r_arg, r_cmd, groups, r_grp)
    _close(d_arg, r_arg, 2e-5, "scatter arg")
    _close(d_cmd, r_cmd, 2e-5, "scatter cmd")
    _close(d_grp, r_grp, 2e-5, "scatter grp")


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_pos_mean_bcast(gpu_device, dtype):
    n_seq, S, d = 70, 31, 256
    seed = _seed_tensor(42)
    pos = _rand(40, d, seed=1)
    x = _rand(n_seq * S, d, dtype=dtype, seed=2)
    tol = 1e-6 if dtype == torch.float32 else 8e-3
    for xx in (x, None):
        for p in (0.0, 0.1):
            y = ops.add_pos_fwd(xx, pos, n_seq, S, dtype, p, 5, seed)
            _close(y, R.add_pos_fwd(xx, pos, n_seq, S, torch.float32, p, 5, seed), tol, "add_pos fwd")
            dy = _rand(n_seq * S, d, dtype=dtype, seed=3)
            dpos, dposr = torch.empty(S, d, device=DEV), torch.empty(S, d, device=DEV)
            dx = ops.add_pos_bwd(dy, n_seq, S, dpos, want_dx=xx is not None, drop_p=p, drop_site=5, seed=seed)
            dxr = R.add_pos_bwd(dy, n_seq, S, dposr, want_dx=xx is not None, drop_p=p, drop_site=5, seed=seed)
            _close(dpos, dposr, 2e-5 if dtype == torch.float32 else 1e-2, "add_pos dpos")
            if xx is not None:
                _close(dx, dxr, tol, "add_pos dx")
    km = _key_masks(n_seq, S, 7)
    m = ops.masked_mean_fwd(x, km, n_seq, S)
    _close(m, R.masked_mean_fwd(x.float(), km, n_seq, S), tol * 4, "masked mean")
    dm = _rand(n_seq, d, dtype=dtype, seed=4)
    _close(ops.masked_mean_bwd(dm, km, n_seq, S), R.masked_mean_bwd(dm.float(), km, n_seq, S), tol, "masked mean bwd")
    g = _rand(n_seq, d, dtype=dtype, seed=5)
    for p in (0.0, 0.1):
        x1, x2 = x.clone(), x.clone().float()
        ops.bcast_add_fwd_(x1, g, n_seq, S, p, 6, seed)
        R.bcast_add_fwd_(x2, g.float(), n_seq, S, p, 6, seed)
        _close(x1, x2, tol, "bcast add")
        _close(ops.bcast_add_bwd(x, n_seq, S, p, 6, seed), R.bcast_add_bwd(x.float(), n_seq, S, p, 6, seed),
               2e-5 if dtype == torch.float32 else 1e-2, "bcast add bwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_targets_and_masked_ce(gpu_device, dtype):
    from deepsvg_amd.svgtensor import CMD_ARGS_MASK
    c, a = _cmd_args(9, seed=6)
    tc, ta = c.view(-1, 32).contiguous(), a.view(-1, 32, 11).contiguous()
    cam = CMD_ARGS_MASK.float().to(DEV)
    outs = ops.loss_targets(tc, ta, cam)
    refs = R.loss_targets(tc, ta, cam)
    for o, r, nm in zip(outs, refs, ["cmd_tgt", "cmd_w", "arg_tgt", "arg_w", "vis_tgt"]):
        assert torch.equal(o.cpu(), r.cpu().to(o.dtype)), nm
    # the same in a permuted sequence order (the second decoder stage's visible-first order): token-level outputs follow the
    # permutation, the visibility targets stay where they were
    perm = torch.randperm(tc.shape[0], generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
    outs_p = ops.loss_targets(tc, ta, cam, seq_perm=perm)
    refs_p = R.loss_targets(tc, ta, cam, seq_perm=perm)
    for o, r, nm in zip(outs_p, refs_p, ["cmd_tgt", "cmd_w", "arg_tgt", "arg_w", "vis_tgt"]):
        assert torch.equal(o.cpu(), r.cpu().to(o.dtype)), "permuted " + nm
    assert torch.equal(outs_p[0], outs[0][perm.long()]) and torch.equal(outs_p[4], outs[4])
    cmd_tgt, cmd_w, arg_tgt, arg_w, vis_tgt = outs
    n_tok = cmd_tgt.numel()
    for (logits, tgt, w, C_, group) in [
            (_rand(n_tok, 7, dtype=dtype, seed=1), cmd_tgt.view(-1), cmd_w.view(-1), 7, 1),
            (_rand(n_tok, 11 * 257, dtype=dtype, seed=2), arg_tgt.view(-1), arg_w.view(-1), 257, 11),
            (_rand(vis_tgt.numel(), 2, dtype=dtype, seed=3), vis_tgt, None, 2, 1)]:
        lse, sc = ops.masked_ce_fwd(logits, tgt, w, C_, group)
        lser, scr = R.masked_ce_fwd(logits.float(), tgt, w, C_, group)
        _close(lse, lser, 2e-6, "lse")
        _close(sc, scr, 1e-5, "sum/count")
        gs = torch.tensor([0.7], device=DEV)
        d = ops.masked_ce_bwd(logits, tgt, w, lse, sc, gs, 2.0, C_, group, pad_to=8)
        dr = R.masked_ce_bwd(logits.float(), tgt, w, lser, scr, gs, 2.0, C_, group, pad_to=8)
        assert d.stride(0) % 8 == 0
        _close(d, dr, 2e-6 if dtype == torch.float32 else 1e-2, "dlogits")


@pytest.mark.parametrize("group", [11, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compact_ce_backward_live_rows_scatter(gpu_device, dtype, group):
    """argument-head backward on the loss-carrying tokens only: token list, compact dlogits, row scatter (bf16 rows of
    16-byte-aligned stride: the wave-per-token kernel; group 6 = the slot range that carries loss without arcs)"""
    n_tok, C_ = 700, 257
    g = torch.Generator().manual_seed(4)
    w = (torch.rand(n_tok, group, generator=g) < 0.15).float()
    w[torch.rand(n_tok, generator=g) < 0.6] = 0.0            # most tokens carry no loss at all
    w = w.to(DEV).view(-1).contiguous()
    live, count = ops.live_rows(w, group)
    elive, ecount = R.live_rows(w, group)
    assert torch.equal(live, elive) and torch.equal(count, ecount)
    n_live = int(count)
    assert 0 < n_live < n_tok
    ld = (group * C_ + 7) // 8 * 8
    buf = _rand(n_tok, ld, dtype=dtype, seed=90)
    logits = buf[:, :group * C_]
    target = torch.randint(0, C_, (n_tok * group,), generator=g).to(torch.int32).to(DEV)
    lse, sc = ops.masked_ce_fwd(logits, target, w, C_, group)
    gs = torch.tensor([0.7], device=DEV)
    rows = (n_live + 127) // 128 * 128
    idx = live[:rows].contiguous()
    dl = ops.masked_ce_bwd(logits, target, w, lse, sc, gs, 1.0, C_, group, pad_to=8, tok_idx=idx)
    ref = R.masked_ce_bwd(logits, target, w, lse, sc, gs, 1.0, C_, group, pad_to=8, tok_idx=idx)
    _close(dl, ref, 1e-6 if dtype == torch.float32 else 1e-2, "compact CE bwd")
    assert torch.count_nonzero(dl[n_live:]) == 0
    dense = ops.masked_ce_bwd(logits, target, w, lse, sc, gs, 1.0, C_, group, pad_to=8)
    assert torch.equal(dl[:n_live], dense[live[:n_live].long()])
    # compact LOGITS as well (fused argument head + loss: only the listed tokens' logits exist)
    cbuf = torch.zeros(rows, ld, device=DEV, dtype=dtype)
    cbuf[:n_live] = buf[live[:n_live].long()]
    clog = cbuf[:, :group * C_]
    lse_c, sc_c = ops.masked_ce_fwd(clog, target, w, C_, group, tok_idx=idx)
    rl, rs = R.masked_ce_fwd(clog, target, w, C_, group, tok_idx=idx)
    _close(lse_c, rl, 1e-6 if dtype == torch.float32 else 1e-2, "compact CE fwd lse")
    _close(sc_c, rs, 1e-5, "compact CE fwd sums")
    _close(sc_c, sc, 1e-5, "compact == dense loss sums")
    dl_c = ops.masked_ce_bwd(clog, target, w, lse_c, sc_c, gs, 1.0, C_, group, pad_to=8, tok_idx=idx, logits_compact=True)
    _close(dl_c, dl, 1e-6 if dtype == torch.float32 else 1e-2, "compact-logits CE bwd == compact CE bwd")
    src = _rand(rows, 256, dtype=dtype, seed=91)
    dst = torch.zeros(n_tok, 256, device=DEV, dtype=dtype)
    ops.scatter_rows(src, idx, dst)
    exp = R.scatter_rows(src, idx, torch.zeros_like(dst))
    assert torch.equal(dst, exp)
    back = ops.gather_groups(dst, idx, rows, 1)
    assert torch.equal(back[:n_live], src[:n_live])


def test_optimizer_matches_torch_adamw(gpu_device):
    n = 100003
    p0, g = _rand(n, seed=1), _rand(n, seed=2, scale=3.0)
    p = p0.clone()
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    lr = torch.tensor([1e-3], device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3)
    for it in range(3):
        gi = g * (it + 1)
        ops.advance_step_(step, None)
        nsq = ops.sumsq(gi)
        _close(nsq, (gi.double() ** 2).sum().float().reshape(1), 1e-5, "sumsq")
        ops.adamw_step_(p, gi, m, v, lr, step, gnorm_sq=nsq, max_norm=1.0)
        ref.grad = gi.clone()
        torch.nn.utils.clip_grad_norm_([ref], 1.0)
        opt.step()
        _close(p, ref.data, 2e-6, f"adamw step {it}")
    assert step.item() == 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_drop_apply_matches_gemm_epilogue_mask(gpu_device, dtype):
    """the mask replayed by drop_apply must be the mask the GEMM epilogue applied (same element ids)"""
    T, N, K = 520, 256, 64
    seed = _seed_tensor(0x1122334455667788)
    x, w = _rand(T, K, dtype=dtype, seed=1), _rand(N, K, dtype=dtype, seed=2)
    y0 = ops.gemm(x, w)
    y1 = ops.gemm(x, w, drop_p=0.25, drop_site=17, seed=seed)
    keep_gemm = (y1.float() != 0) | (y0.float() == 0)
    ones = torch.ones(T, N, device=DEV, dtype=dtype)
    m = ops.drop_apply(ones, 0.25, 17, seed)
    mr = R.drop_apply(ones, 0.25, 17, seed)
    assert torch.equal(m, mr)
    assert torch.equal(m.float() != 0, keep_gemm)
    frac = (m.float() == 0).float().mean().item()
    assert abs(frac - 0.25) < 0.01, frac


def test_cast_gate_add(gpu_device):
    src = _rand(300, 77, seed=1)
    dst, dst_t = torch.empty(300, 77, device=DEV, dtype=torch.bfloat16), torch.empty(77, 300, device=DEV, dtype=torch.bfloat16)
    ops.cast_weights(src, dst, dst_t)
    assert torch.equal(dst, src.to(torch.bfloat16)) and torch.equal(dst_t, src.t().to(torch.bfloat16))
    for dtype in DTYPES:
        a, b = _rand(1000, 16, dtype=dtype, seed=2), _rand(1000, 16, dtype=dtype, seed=3)
        _close(ops.gate_mul(a, b, 1.5), R.gate_mul(a, b, 1.5), 1e-6 if dtype == torch.float32 else 8e-3, "gate_mul")
        _close(ops.add(a, b), R.add(a, b), 1e-6 if dtype == torch.float32 else 8e-3, "add")


# ---------------------------------------------------------------------------------------------------------------
# Hungarian self-matching (deepsvg/model/model.py:311-350)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_match_costs_and_assignment(gpu_device, dtype):
    from deepsvg_amd.synthetic import make_batch
    from deepsvg_amd.svgtensor import CMD_ARGS_MASK
    N, G, S, A, C, n_cmd = 24, 8, 30, 11, 257, 7
    commands, args = make_batch(N, G=G, S=S, seed=77)                    # (N, G, S+2)
    commands[0, :, 1:] = 4                                               # an icon without any visible group
    commands[1, 3, 1:] = 4                                               # an invisible group between visible ones
    S1 = S + 2
    Sd = S1 - 1
    gen = torch.Generator().manual_seed(5)
    ld_a = (A * C + 7) // 8 * 8
    abuf = torch.randn(N * G * Sd, ld_a, generator=gen) * 2
    cbuf = torch.randn(N * G * Sd, 8, generator=gen)
    vbuf = torch.randn(N * G, 8, generator=gen)
    al, cl, vl = (t.to(dtype) for t in (abuf, cbuf, vbuf))
    cam = CMD_ARGS_MASK.float()
    want_cost, want_vis = R.match_costs(cl[:, :n_cmd].float(), al[:, :A * C].float(), vl[:, :2].float(), commands, args,
                                        cam, N, G, G, A, C, n_cmd, 4)
    cost, vis = ops.match_costs(cl.to(DEV)[:, :n_cmd], al.to(DEV)[:, :A * C], vl.to(DEV)[:, :2], commands.to(DEV),
                                args.to(DEV), cam.to(DEV), N, G, G, A, C, n_cmd, 4)
    assert torch.equal(vis.cpu(), want_vis)
    m = want_vis.bool()
    _close(cost.cpu()[m], want_cost[m], 2e-4 if dtype == torch.float32 else 2e-3, "match costs (visible rows)")
    assign, idx, inv = ops.match_assign(cost, vis)
    ref_assign, ref_idx, ref_inv = R.match_assign(cost.cpu(), vis.cpu())
    assert torch.equal(assign.cpu(), ref_assign), "exhaustive search differs from scipy's Hungarian solver"
    assert torch.equal(idx.cpu(), ref_idx) and torch.equal(inv.cpu(), ref_inv)
    assert assign[0].tolist() == list(range(G))                          # nothing visible: identity
    # random cost matrices, every visibility pattern
    gen = torch.Generator().manual_seed(6)
    cost2 = torch.rand(256, G, G, generator=gen)
    vis2 = (torch.arange(256).unsqueeze(1) >> torch.arange(G).unsqueeze(0)) & 1
    a2, i2, v2 = ops.match_assign(cost2.to(DEV), vis2.to(torch.int32).to(DEV))
    r2, ri2, rv2 = R.match_assign(cost2, vis2.to(torch.int32))
    assert torch.equal(a2.cpu(), r2) and torch.equal(i2.cpu(), ri2) and torch.equal(v2.cpu(), rv2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_argmax_rows(gpu_device, dtype):
    """arg-max over class slots stored like the masked-CE operand (row-padded buffer, 11 x 257 slots per token)"""
    T, A, C, ld = 777, 11, 257, 2832
    buf = _rand(T, ld, dtype=dtype, seed=3)
    buf[5, 3 * C + 7] = buf[5, 3 * C + 200] = 100.0           # a tie: the lowest class wins
    got = ops.argmax_rows(buf[:, :A * C], C, A)
    want = R.argmax_rows(buf[:, :A * C].cpu(), C, A)
    assert torch.equal(got.cpu(), want)
    assert int(got[5 * A + 3]) == 7
    cl = _rand(T, 8, dtype=dtype, seed=4)
    assert torch.equal(ops.argmax_rows(cl[:, :7], 7).cpu(), R.argmax_rows(cl[:, :7].cpu(), 7))


# ---------------------------------------------------------------------------------------------------------------
# sequences of more than 64 tokens (csrc/long_seq.hip)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,n_seq,masked,causal", [(65, 5, True, False), (100, 4, False, True), (242, 6, True, False),
                                                   (241, 5, True, True), (256, 3, False, False), (130, 7, True, True)])
def test_attention_long(gpu_device, dtype, S, n_seq, masked, causal):
    H = 8
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=S + 60)
    lens = None
    if masked:
        g = torch.Generator().manual_seed(S)
        lens = torch.randint(1, S + 1, (n_seq,), generator=g).to(torch.int32)
        lens[0], lens[-1] = S, 1
        lens = lens.to(DEV)
    scale = 32 ** -0.5
    seed = _seed_tensor(0x13572468ACE02468)
    for p in (0.0, 0.1):
        o = ops.attention_fwd(qkv, lens, n_seq, S, H, scale, p, 29, seed, causal=causal)
        orf = R.attention_fwd(qkv.float(), lens, n_seq, S, H, scale, p, 29, seed, causal=causal)
        _close(o, orf, 5e-6 if dtype == torch.float32 else 1.5e-2, f"long attn fwd S={S} p={p}")
        do = _rand(n_seq * S, 32 * H, dtype=dtype, seed=S + 61)
        dq = ops.attention_bwd(qkv, lens, do, n_seq, S, H, scale, p, 29, seed, causal=causal)
        dqr = R.attention_bwd(qkv.float(), lens, do.float(), n_seq, S, H, scale, p, 29, seed, causal=causal)
        _close(dq, dqr, 2e-5 if dtype == torch.float32 else 2e-2, f"long attn bwd S={S} p={p}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_sequence_masks_mean_and_targets(gpu_device, dtype):
    from deepsvg_amd.synthetic import make_batch_onestage
    from deepsvg_amd.svgtensor import CMD_ARGS_MASK
    n, T = 9, 240
    commands, args = make_batch_onestage(n, total_len=T, seed=4)
    commands[0, 0, 1:] = 4                                   # EOS right after SOS
    commands[1, 0, :] = 2
    commands[1, 0, 0] = 5                                    # no EOS at all
    S = T + 2
    cmd = commands.view(n, S).to(DEV)
    lens, vis, gm = ops.build_masks(cmd, S, 0, 4)
    want, _, _ = R.build_masks(cmd.cpu(), S, 0, 4)
    assert vis is None and gm is None and lens.dtype == torch.int32 and torch.equal(lens.cpu(), want)
    assert int(lens[0]) == 1 and int(lens[1]) == S
    x = _rand(n * S, 256, dtype=dtype, seed=9)
    _close(ops.masked_mean_fwd(x, lens, n, S), R.masked_mean_fwd(x.float().cpu(), want, n, S).to(DEV),
           1e-6 if dtype == torch.float32 else 1e-2, "prefix mean fwd")
    dz = _rand(n, 256, dtype=dtype, seed=10)
    _close(ops.masked_mean_bwd(dz, lens, n, S), R.masked_mean_bwd(dz.float().cpu(), want, n, S).to(DEV),
           1e-6 if dtype == torch.float32 else 1e-2, "prefix mean bwd")
    if dtype == torch.float32:
        tc = commands.view(n, S).to(DEV)
        ta = args.view(n, S, 11).to(DEV)
        got = ops.loss_targets(tc, ta, CMD_ARGS_MASK.float().to(DEV), 4)
        ref = R.loss_targets(tc.cpu(), ta.cpu(), CMD_ARGS_MASK.float(), 4)
        for a, b, name in zip(got, ref, ("cmd_tgt", "cmd_w", "arg_tgt", "arg_w", "vis_tgt")):
            assert torch.equal(a.cpu().reshape(-1).float(), b.reshape(-1).float()), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_long_single_row_step(gpu_device, dtype):
    """incremental decoding on long sequences: the newest query row alone == that row of the full causal forward"""
    H, S, n_seq = 8, 241, 6
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=91)
    lens = torch.tensor([241, 1, 77, 200, 5, 130], dtype=torch.int32, device=DEV)
    full = ops.attention_fwd(qkv, lens, n_seq, S, H, 32 ** -0.5, causal=True).view(n_seq, S, -1)
    for row in (0, 3, 64, 150, 240):
        buf = torch.full((n_seq * S, 32 * H), 7.0, dtype=dtype, device=DEV)
        ops.attention_fwd(qkv, lens, n_seq, S, H, 32 ** -0.5, causal=True, only_row=row, out=buf)
        got = buf.view(n_seq, S, -1)
        _close(got[:, row], full[:, row], 5e-6 if dtype == torch.float32 else 1e-2, f"row {row}")
        mask = torch.ones(S, dtype=torch.bool, device=DEV)
        mask[row] = False
        assert bool((got[:, mask] == 7.0).all()), "only_row wrote other rows"


# ----------------------------------------------------------------------------------------------------
# fused FFN sub-block (csrc/ffn_fused.hip)
# ----------------------------------------------------------------------------------------------------
FFN_LAYER_PARAMS = 131072 + 512 + 131072 + 256 + 256 + 8     # W1, b1, W2, gamma, beta (+ padding)


def _ffn_setup(rows, seed=0, n_layers=2):
    """fp32 'master' buffer with n_layers x (linear1.weight, linear1.bias, linear2.weight, norm.weight, norm.bias), the
    offsets table dsvg_ffn_pack takes, a bf16 activation matrix and linear2's bias"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat = torch.zeros(8 + n_layers * FFN_LAYER_PARAMS)
    offs = []
    for i in range(n_layers):
        o = 8 + i * FFN_LAYER_PARAMS
        ent = [o, o + 131072, o + 131072 + 512, o + 262144 + 512, o + 262144 + 768]
        flat[ent[0]:ent[0] + 131072] = torch.randn(131072, generator=g) * 0.06
        flat[ent[1]:ent[1] + 512] = torch.randn(512, generator=g) * 0.3
        flat[ent[2]:ent[2] + 131072] = torch.randn(131072, generator=g) * 0.06
        flat[ent[3]:ent[3] + 256] = 1 + 0.2 * torch.randn(256, generator=g)
        flat[ent[4]:ent[4] + 256] = 0.2 * torch.randn(256, generator=g)
        offs.append(ent)
    x = (torch.randn(rows, 256, generator=g) * 1.5 + 0.3).to(DEV).to(torch.bfloat16)
    b2 = (0.3 * torch.randn(256, generator=g)).to(DEV)
    return flat.to(DEV), torch.tensor(offs, dtype=torch.int64, device=DEV), x, b2


def _ffn_params(flat, offs, layer):
    o1, ob1, o2, og, ob = (int(v) for v in offs[layer])
    return (flat[o1:o1 + 131072].view(512, 256), flat[ob1:ob1 + 512], flat[o2:o2 + 131072].view(256, 512),
            flat[og:og + 256], flat[ob:ob + 256])


def test_bcast_add_bwd_with_the_masked_copy(gpu_device):
    """dsvg_bcast_add_bwd_masked: the per-sequence sum AND drop_apply(dx, mask_site) from one read of dx - both bit-identical to
    the two separate launches, incl. a sequence count that does not fill the last workgroup and zero rows past the live prefix"""
    g = torch.Generator(device="cpu").manual_seed(5)
    seed = _seed_tensor(0x5151515151)
    for n_seq, S, n_out, extra in ((37, 31, 37, 0), (64, 8, 80, 0), (5, 3, 5, 0), (37, 31, 64, 133), (3, 31, 5, 62)):
        # (extra: rows past the summed sequences - a live row prefix rounded up - that are masked but not summed)
        dx = torch.randn(n_seq * S + extra, 256, generator=g).to(DEV).to(torch.bfloat16)
        dg0 = ops.bcast_add_bwd(dx, n_seq, S, 0.1, 402, seed, n_seq_out=n_out)
        dm0 = ops.drop_apply(dx, 0.1, 401, seed)
        dg1, dm1 = ops.bcast_add_bwd(dx, n_seq, S, 0.1, 402, seed, n_seq_out=n_out, mask_site=401)
        assert torch.equal(dg0, dg1) and torch.equal(dm0, dm1)
        eg, em = R.bcast_add_bwd(dx, n_seq, S, 0.1, 402, seed, n_seq_out=n_out, mask_site=401)
        assert torch.equal(dm1, em)
        _close(dg1, eg, 1e-2, "bcast_add_bwd (masked variant) dg")
        # ABI 9: dg as a column block of a wider buffer (the layers of a decoder stack write side by side: no concatenation launch)
        wide = torch.full((n_out, 1024), 7.0, dtype=torch.bfloat16, device=DEV)
        r2, m2 = ops.bcast_add_bwd(dx, n_seq, S, 0.1, 402, seed, n_seq_out=n_out, mask_site=401, out=wide[:, 512:768])
        r3 = ops.bcast_add_bwd(dx, n_seq, S, 0.1, 402, seed, n_seq_out=n_out, out=wide[:, 256:512])
        assert r2.data_ptr() == wide[:, 512:768].data_ptr() and torch.equal(wide[:, 512:768], dg0) and torch.equal(m2, dm0)
        assert torch.equal(r3, dg0) and bool((wide[:, :256] == 7.0).all()) and bool((wide[:, 768:] == 7.0).all())


def test_ffn_pack_layouts(gpu_device):
    """every fragment of the packed images against the index formulas of csrc/ffn_fused.hip (lane l = (i, half), 8
    elements e): forward [W1' chunk | W2 chunk], backward [W1' chunk | W2^T chunk | W1'^T chunk], W1' = W1 diag(gamma)
    rounded to bf16 once, and the folded bias b1 + W1 beta"""
    flat, offs, _, _ = _ffn_setup(8, seed=3)
    w2p = torch.empty((2, 256, 512), dtype=torch.bfloat16, device=DEV)
    pf, pb, b1f = ops.ffn_pack(flat, offs, 2, w2p=w2p)
    perm = R._ffn_frag_perm(DEV)
    for layer in range(2):      # linear2.weight with fragment-ordered columns: w2p[:, p(j)] = W2[:, j]
        assert torch.equal(w2p[layer][:, perm], _ffn_params(flat, offs, layer)[2].to(torch.bfloat16))
    pf = pf.view(2, 16, 32, 64, 8).cpu().float()
    pb = pb.view(2, 16, 48, 64, 8).cpu().float()
    lane = torch.arange(64)
    i, half = (lane & 31).view(64, 1), (lane >> 5).view(64, 1)
    e = torch.arange(8).view(1, 8)
    for layer in range(2):
        W1, b1, W2, gamma, beta = (t.cpu() for t in _ffn_params(flat, offs, layer))
        W1g = (W1 * gamma).to(torch.bfloat16).float()
        W2 = W2.to(torch.bfloat16).float()
        assert torch.allclose(b1f[layer].cpu(), b1 + W1 @ beta, rtol=1e-5, atol=1e-5)
        for c in (0, 7, 15):
            for ks in range(16):
                want = W1g[32 * c + i, 16 * ks + 8 * half + e]
                assert torch.equal(pf[layer, c, ks], want) and torch.equal(pb[layer, c, ks], want)
                assert torch.equal(pb[layer, c, 16 + ks], W2[16 * ks + 8 * half + e, 32 * c + i])
            for t in range(8):
                for ks2 in range(2):
                    hid = (e & 3) + 8 * (2 * ks2 + (e >> 2)) + 4 * half
                    assert torch.equal(pf[layer, c, 16 + 2 * t + ks2], W2[32 * t + i, 32 * c + hid])
                    assert torch.equal(pb[layer, c, 32 + 2 * t + ks2], W1g[32 * c + hid, 32 * t + i])


@pytest.mark.parametrize("rows", [256, 1000, 4096 + 37])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_ffn_fwd_matches_reference(gpu_device, rows, drop_p):
    """fused LayerNorm + linear1 + ReLU + dropout + linear2 + dropout + residual against the fp32 restatement (same
    bf16 rounding points: normalised rows, folded weights, hidden activations), incl. ragged row counts and the
    dropout replay"""
    flat, offs, x, b2 = _ffn_setup(rows, seed=rows)
    pf, pb, b1f = ops.ffn_pack(flat, offs, 2)
    epf, _, eb1f = R.ffn_pack(flat, offs, 2)
    _close(b1f, eb1f.to(b1f.device), 1e-5, "folded linear1 bias (b1 + W1 beta)")
    seed = _seed_tensor(0x0123456789ABCDEF)
    for layer in (0, 1):
        sl = slice(layer * ops.FFN_FWD_LAYER_ELEMS, (layer + 1) * ops.FFN_FWD_LAYER_ELEMS)
        y = ops.ffn_fwd(x, pf[sl], b1f[layer], b2, 1e-5, drop_p, 403 + layer, 404 + layer, seed)
        want = R.ffn_fwd(x, epf[sl], eb1f[layer], b2, 1e-5, drop_p, 403 + layer, 404 + layer, seed)
        _close(y, want, 1.5e-2, f"ffn_fwd rows={rows} p={drop_p} layer={layer}")
        # rounding-level agreement on the bulk, not just the max
        assert (y.float() - want.float()).abs().mean().item() < 2e-3 * want.float().abs().mean().item()
    # training call: same y, plus h (fragment order), xh and rstd for the backward pass
    pl = pf[:ops.FFN_FWD_LAYER_ELEMS]
    y0 = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed)
    yt, h, xh, rstd = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed, train=True)
    wy, wh, wxh, wrstd = R.ffn_fwd(x, epf[:ops.FFN_FWD_LAYER_ELEMS], eb1f[0], b2, 1e-5, drop_p, 403, 404, seed, train=True)
    assert torch.equal(yt, y0)
    same = (h != 0) == (wh != 0)        # ReLU gates within rounding of zero may differ (other fp32 summation order)
    assert (~same).float().mean().item() < 2e-3
    _close(torch.where(same, h, torch.zeros_like(h)), torch.where(same, wh, torch.zeros_like(wh)), 1.5e-2, "ffn_fwd train h")
    _close(xh, wxh, 1.5e-2, "ffn_fwd train xh")
    assert torch.allclose(rstd, wrstd, rtol=1e-4, atol=1e-6)
    if drop_p > 0:      # the masks are a pure function of (seed, site, id): another seed gives another output
        pl = pf[:ops.FFN_FWD_LAYER_ELEMS]
        y1 = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, _seed_tensor(7))
        y2 = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, _seed_tensor(7))
        y3 = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, _seed_tensor(8))
        assert torch.equal(y1, y2) and not torch.equal(y1, y3)


@pytest.mark.parametrize("rows", [100, 4096 + 37, 40000])
def test_ffn_fwd_workgroup_variants_agree(gpu_device, rows):
    """the 256-row workgroups (3- and 4-slot weight rings) and the half-size workgroups (128 rows, the default up to
    32,768 rows) run the same per-wave program: every output is bit-identical, inference and training variants - once with the
    scalar activation code (stages 2 / 3 / 4) and once with the packed one (stages 7 / 6 and the default)"""
    flat, offs, x, b2 = _ffn_setup(rows, seed=rows + 1)
    pf, _, b1f = ops.ffn_pack(flat, offs, 2)
    pl = pf[:ops.FFN_FWD_LAYER_ELEMS]
    seed = _seed_tensor(0x1122334455667788)
    for train in (False, True):
        outs = {}
        for stages in (2, 3, 4, 6, 7, None):
            r = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, 0.1, 403, 404, seed, train=train, stages=stages)
            outs[stages] = r if train else (r,)
        for ref, others in ((2, (3, 4)), (7, (6, None))):
            for stages in others:
                for a, b in zip(outs[ref], outs[stages]):
                    assert torch.equal(a, b), (rows, train, stages)


def _bf16_steps(a, b):
    """distance of two bf16 tensors in representable steps (order-preserving integer image of the bit patterns)"""
    ai, bi = a.view(torch.int16).to(torch.int32), b.view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -32768 - ai, ai)
    bi = torch.where(bi < 0, -32768 - bi, bi)
    return (ai - bi).abs()


@pytest.mark.parametrize("rows", [100, 128, 1000, 4096 + 37, 40000])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_ffn_fwd_packed_variant(gpu_device, rows, drop_p):
    """round 5: the packed activation (stages 6) against the scalar 256-row kernel (stages 4).  Same dropout draws (the
    kept / dropped elements of h are the same elements), same xh / rstd bits; h and y differ by fp32 summation order
    before the bf16 rounding: h within ONE bf16 step wherever it is not within rounding of zero, y as close to the
    restatement as the scalar kernel is.
    stages = 5 (the role-specialised kernel, removed) is an error, not a silent run of another kernel"""
    flat, offs, x, b2 = _ffn_setup(rows, seed=rows + 7)
    pf, _, b1f = ops.ffn_pack(flat, offs, 2)
    epf, _, eb1f = R.ffn_pack(flat, offs, 2)
    pl = pf[:ops.FFN_FWD_LAYER_ELEMS]
    seed = _seed_tensor(0x0BADC0FFEE123457)
    want = R.ffn_fwd(x, epf[:ops.FFN_FWD_LAYER_ELEMS], eb1f[0], b2, 1e-5, drop_p, 403, 404, seed)
    y4, h4, xh4, rstd4 = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed, train=True, stages=4)
    e4 = (y4.float() - want.float()).abs().max().item()
    scale = want.float().abs().max().item()
    for stages in (6,):
        y, h, xh, rstd = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed, train=True, stages=stages)
        yi = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed, stages=stages)
        assert torch.equal(y, yi), "training and inference variants compute the same y"
        assert torch.equal(xh, xh4) and torch.equal(rstd, rstd4)
        same_gate = (h != 0) == (h4 != 0)
        assert (~same_gate).float().mean().item() < 1e-4, stages        # pre-activations within fp32 rounding of zero
        steps = _bf16_steps(h, h4)
        big = (h4.float().abs() > 1e-2) & same_gate
        assert int(steps[big].max().item()) <= 1, (stages, int(steps[big].max().item()))
        assert (steps != 0).float().mean().item() < 2e-3
        e = (y.float() - want.float()).abs().max().item()
        assert e <= max(1.5e-2 * scale, 1.5 * e4), (stages, e, e4)
        assert (y.float() - y4.float()).abs().mean().item() < 2e-4 * y4.float().abs().mean().item()
    if rows == 100:
        with pytest.raises(lib.DsvgError, match=r"stages must be one of 0, 2, 3, 4, 6, 7"):
            ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed, stages=5)


def test_ffn_fwd_equals_unfused_kernels(gpu_device):
    """eval mode: the fused kernel against the three launches it replaces (layernorm_fwd + 2 GEMMs on the bf16 weights);
    the fused path rounds W1 diag(gamma) and the un-scaled normalised rows to bf16 instead of W1 and the scaled rows"""
    rows = 2048
    flat, offs, x, b2 = _ffn_setup(rows, seed=11)
    pf, _, b1f = ops.ffn_pack(flat, offs, 2)
    W1, b1, W2, gamma, beta = _ffn_params(flat, offs, 0)
    xn, _, _ = ops.layernorm_fwd(x, gamma.contiguous(), beta.contiguous())
    h = ops.gemm(xn, W1.to(torch.bfloat16), bias=b1.contiguous(), act=ops.RELU)
    want = ops.gemm(h, W2.to(torch.bfloat16), bias=b2, res=x)
    y = ops.ffn_fwd(x, pf[:ops.FFN_FWD_LAYER_ELEMS], b1f[0], b2)
    _close(y, want, 1.2e-2, "fused vs unfused FFN")


def _ffn_step_bwd(x, dy, pf_layer, pb_layer, b1f_layer, b2, w2p_layer, drop_p, site_h, site_r, seed):
    """the FFN sub-block's backward as a training step runs it: ffn_fwd(train=True) for h / xh, then drop_apply -> gated GEMM
    on W2p -> ffn_bwd_dx.  -> (dx, h, dpre, xh, dym), h / dpre in fragment order (the tuple R.ffn_bwd returns)"""
    _, h, xh, _ = ops.ffn_fwd(x, pf_layer, b1f_layer, b2, 1e-5, drop_p, site_h, site_r, seed, train=True)
    dym = ops.drop_apply(dy, drop_p, site_r, seed)
    dpre = ops.gemm(dym, w2p_layer, b_kc=False, gate=h, gate_scale=1.0 / (1.0 - drop_p))
    dx = ops.ffn_bwd_dx(dpre, x, dy, pb_layer)
    return dx, h, dpre, xh, dym


@pytest.mark.parametrize("rows", [256, 1000, 4096 + 37])
@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_ffn_bwd_matches_reference(gpu_device, rows, drop_p):
    """the step's backward sequence (_ffn_step_bwd: training forward, drop_apply, gated GEMM, ffn_bwd_dx) against the
    restatement: dx, and the operands handed to the weight-gradient GEMMs (h / dpre in fragment order, xh, dym), with both
    dropout masks replayed from the forward's ids"""
    flat, offs, x, b2 = _ffn_setup(rows, seed=rows + 1)
    w2p = torch.empty((2, 256, 512), dtype=torch.bfloat16, device=DEV)
    pf, pb, b1f = ops.ffn_pack(flat, offs, 2, w2p=w2p)
    _, epb, eb1f = R.ffn_pack(flat, offs, 2)
    g = torch.Generator(device="cpu").manual_seed(rows)
    dy = torch.randn(rows, 256, generator=g).to(DEV).to(torch.bfloat16)
    seed = _seed_tensor(0x0123456789ABCDEF)
    sl = slice(ops.FFN_BWD_LAYER_ELEMS, 2 * ops.FFN_BWD_LAYER_ELEMS)
    got = _ffn_step_bwd(x, dy, pf[ops.FFN_FWD_LAYER_ELEMS:], pb[sl], b1f[1], b2, w2p[1], drop_p, 403, 404, seed)
    want = R.ffn_bwd(x, dy, epb[sl], eb1f[1], 1e-5, drop_p, 403, 404, seed)
    # ReLU gates of units whose pre-activation is within rounding of zero may differ between kernel and restatement
    # (a different fp32 summation order): compare h / dpre where both agree on the gate, and bound the disagreements
    gate_k, gate_r = got[1] != 0, want[1] != 0
    if drop_p == 0:
        same = gate_k == gate_r
        assert (~same).float().mean().item() < 2e-3
    else:       # (a dropped unit is zero in both)
        same = gate_k == gate_r
        assert (~same).float().mean().item() < 2e-3
    for name, a, b in zip(("dx", "h", "dpre", "xh", "dym"), got, want):
        if name in ("h", "dpre"):
            a, b = torch.where(same, a, torch.zeros_like(a)), torch.where(same, b, torch.zeros_like(b))
        _close(a, b, 3e-2 if name == "dx" else 1.5e-2, f"ffn_bwd {name} rows={rows} p={drop_p}")
        assert (a.float() - b.float()).abs().mean().item() < 4e-3 * b.float().abs().mean().item() + 1e-6, name
    if drop_p > 0:      # forward and backward draw the same masks: where the forward zeroed h, dpre is zero too
        y = ops.ffn_fwd(x, pf[ops.FFN_FWD_LAYER_ELEMS:], b1f[1], b2, 1e-5, drop_p, 403, 404, seed)
        assert torch.equal(got[1] == 0, got[2] == 0) or ((got[1] == 0) != (got[2] == 0)).float().mean().item() < 1e-3
        assert (got[4] == 0).float().mean().item() > 0.08 and y.isfinite().all()


def test_ffn_bwd_dx_masked_second_output(gpu_device):
    """dsvg_ffn_bwd_dx can hand back dx with a dropout mask replayed on it from the same launch: bit-identical to
    dsvg_drop_apply on its first output (same ids row * 256 + column, applied to the bf16-rounded dx)"""
    rows = 4133
    flat, offs, x, _ = _ffn_setup(rows, seed=9)
    _, pb, _ = ops.ffn_pack(flat, offs, 2)
    dpre = (_rand(rows, 512, seed=91) * 0.3).to(torch.bfloat16)
    dy = _rand(rows, 256, seed=92).to(torch.bfloat16)
    seed = _seed_tensor(0x00C0FFEE12345678)
    layer = pb[ops.FFN_BWD_LAYER_ELEMS:2 * ops.FFN_BWD_LAYER_ELEMS]
    dx0 = ops.ffn_bwd_dx(dpre, x, dy, layer)
    dx, dxm = ops.ffn_bwd_dx(dpre, x, dy, layer, masked=(0.1, 77, seed))
    assert torch.equal(dx, dx0)
    assert torch.equal(dxm, ops.drop_apply(dx0, 0.1, 77, seed))
    assert 0.05 < (dxm == 0).float().mean().item() < 0.15
    dx2, dxm2 = ops.ffn_bwd_dx(dpre, x, dy, layer, masked=(0.0, 77, seed))
    assert torch.equal(dx2, dx0) and dxm2 is dx2


def test_ffn_wgrad_finish_and_full_gradients(gpu_device):
    """fused forward + backward + the two weight-gradient GEMMs + wgrad_finish against autograd on the unfused fp32
    formulation (LayerNorm with gamma / beta, linear1, ReLU, linear2, residual; no dropout): dx, dW1, db1, dW2, db2,
    dgamma, dbeta"""
    rows = 3000
    flat, offs, x, b2 = _ffn_setup(rows, seed=5)
    w2p = torch.empty((2, 256, 512), dtype=torch.bfloat16, device=DEV)
    pf, pb, b1f = ops.ffn_pack(flat, offs, 2, w2p=w2p)
    W1, b1, W2, gamma, beta = (t.clone().requires_grad_(True) for t in _ffn_params(flat, offs, 0))
    g = torch.Generator(device="cpu").manual_seed(9)
    dy = torch.randn(rows, 256, generator=g).to(DEV).to(torch.bfloat16)
    xf = x.float().requires_grad_(True)
    xn = torch.nn.functional.layer_norm(xf, (256,), gamma, beta, 1e-5)
    yref = xf + torch.relu(xn @ W1.t() + b1) @ W2.t() + b2
    yref.backward(dy.float())
    dx, h, dpre, xh, dym = _ffn_step_bwd(x, dy, pf[:ops.FFN_FWD_LAYER_ELEMS], pb[:ops.FFN_BWD_LAYER_ELEMS], b1f[0], b2,
                                         w2p[0], 0.0, 0, 0, None)
    g2p = torch.empty(256, 512, device=DEV)
    g1p = torch.empty(512, 256, device=DEV)
    db1p, db2 = torch.empty(512, device=DEV), torch.empty(256, device=DEV)
    ops.gemm(dym, h, a_kc=False, b_kc=False, out=g2p, split_k=ops.split_k_for(256, 512, rows), rowsum=db2)
    ops.gemm(dpre, xh, a_kc=False, b_kc=False, out=g1p, split_k=ops.split_k_for(512, 256, rows), rowsum=db1p)
    outs = [torch.empty(n, device=DEV) for n in (131072, 512, 131072, 256, 256)]
    ops.ffn_wgrad_finish(g1p, db1p, g2p, W1.detach().contiguous(), gamma.detach().contiguous(),
                         beta.detach().contiguous(), *outs)
    dw1, db1, dw2, dgamma, dbeta = outs
    # emulated wgrad_finish agrees bit for bit on the same inputs (pure fp32 elementwise + fixed-order sums aside)
    eouts = [torch.empty_like(t) for t in outs]
    R.ffn_wgrad_finish(g1p, db1p, g2p, W1.detach(), gamma.detach(), beta.detach(), *eouts)
    for a, b in zip(outs, eouts):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)
    # the batched launch (all fused-FFN layers of a backward pass at once; 19 layers: two launches of 16 + 3): bit-identical
    layers = []
    for i in range(19):
        o_i = [torch.full_like(t, float("nan")) for t in outs]
        layers.append((g1p * (i + 1), db1p * (i + 1), g2p * (i + 1), W1.detach().contiguous(), gamma.detach().contiguous(),
                       beta.detach().contiguous(), *o_i))
    ops.ffn_wgrad_finish_many(layers)
    for i in (0, 7, 16, 18):
        single = [torch.empty_like(t) for t in outs]
        ops.ffn_wgrad_finish(*layers[i][:6], *single)
        for a, b in zip(layers[i][6:], single):
            assert torch.equal(a, b), f"batched finish differs from the single launch (layer {i})"
    checks = [("dx", dx.float(), xf.grad), ("dW1", dw1.view(512, 256), W1.grad), ("db1", db1, b1.grad),
              ("dW2", dw2.view(256, 512), W2.grad), ("db2", db2, dy.float().sum(0)), ("dgamma", dgamma, gamma.grad),
              ("dbeta", dbeta, beta.grad)]
    for name, a, b in checks:
        rel = ((a - b).norm() / b.norm()).item()
        print(f"{name}: relative L2 error {rel:.3e}")
        # ReLU gates that flip under bf16 rounding of the pre-activation (~0.1 % of the units on this data) put an
        # O(sqrt(flip fraction)) floor under everything downstream of dpre; dW2 / db2 do not depend on the gate
        assert rel < (2e-2 if name in ("dW2", "db2") else 8e-2), (name, rel)


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
def test_ffn_training_path_matches_reference(gpu_device, drop_p):
    """the default training path: forward kernel with train=True (stores h in fragment order + xh), then in the backward
    pass drop_apply -> gated GEMM on W2p -> ffn_bwd_dx; every step against its restatement on the kernel's own h.
    The end-to-end comparison with the fully fused backward kernel went with that kernel: dpre, dx and h of this very path
    are held against the independent restatement R.ffn_bwd by test_ffn_bwd_matches_reference (six cases), dym is bit-equal to
    the restatement below.  The one assertion without a successor is the bit-equality of the two kernels' xh (two
    instantiations of one inline function, one of them deleted): xh keeps its 1.5e-2 bound against the restatement in
    test_ffn_bwd_matches_reference - not bit-equal there, the kernel takes sum / sum of squares where torch takes a two-pass
    variance - and its bit-equality across the forward variants stays in test_ffn_fwd_packed_variant."""
    rows = 2000
    flat, offs, x, b2 = _ffn_setup(rows, seed=21)
    w2p = torch.empty((2, 256, 512), dtype=torch.bfloat16, device=DEV)
    pf, pb, b1f = ops.ffn_pack(flat, offs, 2, w2p=w2p)
    ew2p = torch.empty_like(w2p)
    epf, epb, eb1f = R.ffn_pack(flat, offs, 2, w2p=ew2p)
    assert torch.equal(w2p, ew2p)
    g = torch.Generator(device="cpu").manual_seed(3)
    dy = torch.randn(rows, 256, generator=g).to(DEV).to(torch.bfloat16)
    seed = _seed_tensor(0x0123456789ABCDEF)
    pl, pbl = pf[:ops.FFN_FWD_LAYER_ELEMS], pb[:ops.FFN_BWD_LAYER_ELEMS]
    y, h, xh, rstd = ops.ffn_fwd(x, pl, b1f[0], b2, 1e-5, drop_p, 403, 404, seed, train=True)
    inv_keep = 1.0 / (1.0 - drop_p) if drop_p > 0 else 1.0
    dym = ops.drop_apply(dy, drop_p, 404, seed)
    dpre = ops.gemm(dym, w2p[0], b_kc=False, gate=h, gate_scale=inv_keep)
    dx = ops.ffn_bwd_dx(dpre, x, dy, pbl)
    # restatement of the same three steps on the kernel's own h (the gate)
    edym = R.drop_apply(dy, drop_p, 404, seed)
    edpre = R.gemm(edym, ew2p[0], b_kc=False, gate=h, gate_scale=inv_keep)
    edx = R.ffn_bwd_dx(edpre, x, dy, epb[:ops.FFN_BWD_LAYER_ELEMS])
    assert torch.equal(dym, edym)
    _close(dpre, edpre, 1.5e-2, "training path dpre")
    _close(dx, edx, 2e-2, "training path dx")


def _attn_setup(seed=0, n_layers=2):
    """fp32 'master' buffer with n_layers x (in_proj_weight, out_proj.weight) and the offsets table dsvg_attn_pack takes;
    biases and the LayerNorm affine of the layer under test"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    per = 768 * 256 + 256 * 256
    flat = torch.zeros(8 + n_layers * per)
    offs = []
    for i in range(n_layers):
        o = 8 + i * per
        flat[o:o + 196608] = torch.randn(196608, generator=g) * 0.06
        flat[o + 196608:o + per] = torch.randn(65536, generator=g) * 0.06
        offs.append([o, o + 196608])
    extra = dict(in_bias=0.2 * torch.randn(768, generator=g), out_bias=0.2 * torch.randn(256, generator=g),
                 gamma=1 + 0.2 * torch.randn(256, generator=g), beta=0.2 * torch.randn(256, generator=g))
    return flat.to(DEV), torch.tensor(offs, dtype=torch.int64, device=DEV), {k: v.to(DEV) for k, v in extra.items()}


def test_attn_pack_layout(gpu_device):
    """every fragment of the packed image against the index formulas of csrc/attn_fused.hip"""
    flat, offs, _ = _attn_setup(seed=5)
    img = ops.attn_pack(flat, offs, 2).view(2, 512, 64, 8).cpu().float()
    lane = torch.arange(64)
    i, half = (lane & 31).view(64, 1), (lane >> 5).view(64, 1)
    e = torch.arange(8).view(1, 8)
    for layer in range(2):
        oi, oo = (int(v) for v in offs[layer])
        Win = flat[oi:oi + 196608].view(768, 256).to(torch.bfloat16).float().cpu()
        Wo = flat[oo:oo + 65536].view(256, 256).to(torch.bfloat16).float().cpu()
        for f in (0, 17, 47, 48, 100, 383):
            h, g = f // 48, f % 48
            sel, ks = g >> 4, g & 15
            assert torch.equal(img[layer, f], Win[256 * sel + 32 * h + i, 16 * ks + 8 * half + e]), f
        for f in (384, 385, 399, 400, 470, 511):
            g = f - 384
            t, h, ks2 = g >> 4, (g & 15) >> 1, g & 1
            r = 8 * ks2 + e
            col = 32 * h + (r & 3) + 8 * (r >> 2) + 4 * half
            assert torch.equal(img[layer, f], Wo[32 * t + i, col]), f


def test_attn_pack_bwd_layout(gpu_device):
    """every element of the attention backward image, bit for bit, against the index formula of csrc/pack_images.h:
    img[layer][head h][K step ks][lane l][e] = bf16(Wo[16 ks + 8 (l >> 5) + e][32 h + (l & 31)]), 128 fragments per layer, in
    a caller-provided buffer, and nothing written behind the last layer"""
    flat, offs, _ = _attn_setup(seed=6)
    n = 2 * ops.ATTN_BWD_LAYER_ELEMS
    assert ops.ATTN_BWD_LAYER_ELEMS == 128 * 512
    tail = (torch.arange(512, dtype=torch.int16) + 0x3C00).view(torch.bfloat16).to(DEV)
    buf = torch.zeros(n + 512, dtype=torch.bfloat16, device=DEV)
    buf[n:] = tail
    out = ops.attn_pack_bwd(flat, offs, 2, buf[:n])
    assert out.data_ptr() == buf.data_ptr()
    img = buf[:n].view(2, 8, 16, 64, 8).view(torch.int16).cpu()
    lane = torch.arange(64).view(1, 1, 64, 1)
    h, ks, e = torch.arange(8).view(8, 1, 1, 1), torch.arange(16).view(1, 16, 1, 1), torch.arange(8).view(1, 1, 1, 8)
    for layer in range(2):
        oo = int(offs[layer][1])
        Wo = flat[oo:oo + 65536].view(256, 256).to(torch.bfloat16).view(torch.int16).cpu()
        assert torch.equal(img[layer], Wo[16 * ks + 8 * (lane >> 5) + e, 32 * h + (lane & 31)]), layer
    assert torch.equal(buf[n:].view(torch.int16), tail.view(torch.int16))


def _attn_case(kind, seed):
    """-> (rows, n_seq, S, key_mask, seq_off, tiles, n_real_rows)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "packed":
        n_seq, S = 700, 30
        lens = torch.randint(1, S + 1, (n_seq,), generator=g)
        lens[::7] = torch.randint(1, 6, (len(lens[::7]),), generator=g)         # short sequences: several per tile
        off = torch.zeros(n_seq + 1, dtype=torch.int32)
        off[1:] = lens.cumsum(0)
        real = int(off[-1])
        rows = (real + 255) // 256 * 256 + 64          # bucket padding behind the last sequence
        seq_off = off.to(DEV)
        return rows, n_seq, S, None, seq_off, ops.attention_tiles(seq_off, n_seq, 32), real
    if kind == "dense31":
        return 300 * 31, 300, 31, None, None, None, 300 * 31
    if kind == "dense32_masked":
        n_seq, S = 257, 32
        lens = torch.randint(1, S + 1, (n_seq,), generator=g)
        km = ((torch.ones(n_seq, dtype=torch.int64) << lens) - 1).to(DEV)
        return n_seq * S, n_seq, S, km, None, None, n_seq * S
    if kind == "dense8_masked_tail":
        n_seq, S = 1001, 8            # four sequences per 32-row tile, the last tile holds one
        lens = torch.randint(1, S + 1, (n_seq,), generator=g)
        km = ((torch.ones(n_seq, dtype=torch.int64) << lens) - 1).to(DEV)
        return n_seq * S + 40, n_seq, S, km, None, None, n_seq * S
    if kind == "dense10":           # three sequences per tile (30 of 32 rows)
        return 500 * 10, 500, 10, None, None, None, 500 * 10
    if kind == "tiny_dense5":       # one workgroup, one partly filled tile (3 sequences of 5)
        return 15, 3, 5, None, None, None, 15
    if kind == "one_sequence_32":
        return 32, 1, 32, None, None, None, 32
    if kind == "packed_extremes":   # lengths 1 and 32 mixed: tiles of one full sequence next to tiles of up to 32 singletons
        n_seq, S = 300, 32
        lens = torch.where(torch.rand(n_seq, generator=g) < 0.5, torch.tensor(1), torch.tensor(32))
        lens[40:100] = 1            # 60 singletons in a row
        off = torch.zeros(n_seq + 1, dtype=torch.int32)
        off[1:] = lens.cumsum(0)
        real = int(off[-1])
        seq_off = off.to(DEV)
        return real, n_seq, S, None, seq_off, ops.attention_tiles(seq_off, n_seq, 32), real
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["packed", "dense31", "dense32_masked", "packed_extremes", "one_sequence_32"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_bwd_with_the_out_proj_backward_inside(gpu_device, kind, p):
    """dsvg_attention_bwd_outproj (dO = dx1m . Wo formed per tile on chip) against the two launches it replaces - the
    `dao = dx1m @ Wo` GEMM and dsvg_attention_bwd - and against their fp32 torch restatement"""
    flat, offs, prm = _attn_setup(seed=13)
    rows, n_seq, S, km, seq_off, tiles, real = _attn_case(kind, seed=23)
    qkv = (_rand(rows, 768, seed=33) * 0.8).to(torch.bfloat16)
    dx1m = (_rand(rows, 256, seed=34) * 0.6).to(torch.bfloat16)
    if real < rows:
        dx1m[real:] = 0            # (rows behind the last sequence carry no gradient)
    layer = 1
    oo = int(offs[layer][1])
    wo = flat[oo:oo + 65536].view(256, 256).to(torch.bfloat16)
    img = ops.attn_pack_bwd(flat, offs, 2)
    wob = img[layer * ops.ATTN_BWD_LAYER_ELEMS:(layer + 1) * ops.ATTN_BWD_LAYER_ELEMS]
    eimg = R.attn_pack_bwd(flat, offs, 2)
    assert torch.equal(eimg[layer * R.ATTN_BWD_LAYER_ELEMS:(layer + 1) * R.ATTN_BWD_LAYER_ELEMS][:65536].view(256, 256), wo)
    seed = _seed_tensor(0x0BADC0FFEE12345B)
    scale = 32 ** -0.5
    got = ops.attention_bwd_outproj(qkv, km, dx1m, wob, n_seq, S, scale, p, 7, seed, seq_off=seq_off, tiles=tiles)
    dao = ops.gemm(dx1m, wo, b_kc=False)
    want = ops.attention_bwd(qkv, km, dao, n_seq, S, 8, scale, p, 7, seed, seq_off=seq_off, tiles=tiles)
    ref = R.attention_bwd_outproj(qkv.float(), km, dx1m.float(), wo.float().reshape(-1), n_seq, S, scale, p, 7, seed,
                                  seq_off=seq_off, tiles=tiles)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    r = slice(0, real)
    # the unfused pair rounds dao to bf16 before the attention backward reads it, the fused kernel does too (its staging tile)
    _close(got[r], want[r], 1.5e-2, "dqkv vs GEMM + attention_bwd")
    _close(got[r], ref[r], 2e-2, "dqkv vs fp32 torch")
    assert ((got[r].float() - ref[r].float()).abs().mean() <= 4e-3 * ref[r].float().abs().mean()).item()
    if real < rows:
        assert torch.count_nonzero(got[real:]) == 0


@pytest.mark.parametrize("kind", ["packed", "dense31", "dense32_masked", "dense8_masked_tail", "packed_extremes"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attn_block_fwd_against_fp32_torch(gpu_device, kind, p):
    """the fused attention block DIRECTLY against the plain-torch fp32 restatement (tests/torch_ops_ref.py: LayerNorm,
    in_proj, per-head masked softmax with the replayed dropout draws, out_proj, dropout, residual) run on fp32 copies of the
    same bf16 inputs and weights - no HIP kernel and no bf16 rounding between the steps on the reference side.  Bounds:
    the kernel rounds LN(x), q|k|v, the probabilities and the head outputs to bf16 (2^-9 relative each); worst element
    against the tensor's largest magnitude, mean error against its mean magnitude."""
    flat, offs, prm = _attn_setup(seed=12)
    rows, n_seq, S, km, seq_off, tiles, real = _attn_case(kind, seed=22)
    x = (_rand(rows, 256, seed=32) * 1.5 + 0.3).to(torch.bfloat16)
    img = ops.attn_pack(flat, offs, 2)
    layer = 0
    packed = img[layer * ops.ATTN_LAYER_ELEMS:(layer + 1) * ops.ATTN_LAYER_ELEMS]
    oi, oo = (int(v) for v in offs[layer])
    w32 = torch.cat([flat[oi:oi + 196608], flat[oo:oo + 65536]]).to(torch.bfloat16).float()   # the values the kernel multiplies by
    seed = _seed_tensor(0x0BADC0FFEE123459)
    scale = 32 ** -0.5
    want = R.attn_block_fwd(x.float(), w32, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], km, n_seq, S, scale,
                            1e-5, p, 7, 8, seed, seq_off=seq_off, tiles=tiles, train=True)
    got = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], km, n_seq, S, scale,
                             1e-5, p, 7, 8, seed, seq_off=seq_off, tiles=tiles, train=True)
    torch.cuda.synchronize()
    assert all(w.dtype == torch.float32 for w in want)
    r = slice(0, real)
    for (g, w, tol, mean_tol, what) in zip(got, want, (1.5e-2, 8e-3, 8e-3, 1.5e-2, 1e-5, 1e-5),
                                           (1e-2, 4e-3, 1e-2, 1e-2, 1e-6, 1e-6),
                                           ("x1", "LN(x)", "q|k|v", "head outputs", "mean", "rstd")):
        _close(g[r], w[r], tol, what)
        err = (g[r].float() - w[r]).abs().mean().item()
        ref = w[r].abs().mean().item()
        assert err <= mean_tol * ref + 1e-12, f"{what}: mean abs error {err:.3e} = {err / ref:.2e} of the mean magnitude"


@pytest.mark.parametrize("kind", ["packed", "dense31", "dense32_masked", "dense8_masked_tail", "dense10", "tiny_dense5",
                                  "one_sequence_32", "packed_extremes"])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attn_block_fwd_equals_unfused_kernels(gpu_device, kind, p):
    """the fused attention block against the four launches it replaces (LayerNorm, in_proj GEMM, attention, out_proj GEMM
    with dropout + residual), same weights, same dropout seed and sites: result and every tensor it hands the backward pass.
    Both paths round q|k|v and the head outputs to bf16 at the same points; they differ in fp32 summation order only."""
    flat, offs, prm = _attn_setup(seed=11)
    rows, n_seq, S, km, seq_off, tiles, real = _attn_case(kind, seed=21)
    x = (_rand(rows, 256, seed=31) * 1.5 + 0.3).to(torch.bfloat16)
    img = ops.attn_pack(flat, offs, 2)
    layer = 1
    packed = img[layer * ops.ATTN_LAYER_ELEMS:(layer + 1) * ops.ATTN_LAYER_ELEMS]
    oi, oo = (int(v) for v in offs[layer])
    win = flat[oi:oi + 196608].view(768, 256).to(torch.bfloat16)
    wo = flat[oo:oo + 65536].view(256, 256).to(torch.bfloat16)
    seed = _seed_tensor(0x0BADC0FFEE123457)
    scale = 32 ** -0.5
    # unfused
    xn0, mean0, rstd0 = ops.layernorm_fwd(x, prm["gamma"], prm["beta"], 1e-5)
    qkv0 = ops.gemm(xn0, win, bias=prm["in_bias"])
    ao0 = ops.attention_fwd(qkv0, km, n_seq, S, 8, scale, p, 7, seed, seq_off=seq_off, tiles=tiles)
    want = ops.gemm(ao0, wo, bias=prm["out_bias"], res=x, drop_p=p, drop_site=8, seed=seed)
    # fused
    x1, xn, qkv, ao, mean, rstd = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"],
                                                     km, n_seq, S, scale, 1e-5, p, 7, 8, seed, seq_off=seq_off, tiles=tiles,
                                                     train=True)
    x1i = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], km, n_seq, S, scale,
                             1e-5, p, 7, 8, seed, seq_off=seq_off, tiles=tiles, train=False)
    torch.cuda.synchronize()
    assert torch.equal(x1, x1i), "training and inference variants differ"
    for t in (x1, xn, qkv, ao, mean, rstd):
        assert torch.isfinite(t.float()).all(), "non-finite values (padding rows included)"
    r = slice(0, real)
    _close(mean[r], mean0[r], 1e-5, "mean")
    _close(rstd[r], rstd0[r], 1e-5, "rstd")
    _close(xn[r], xn0[r], 8e-3, "LN(x)")
    _close(qkv[r], qkv0[r], 1.2e-2, "q|k|v")
    _close(ao[r], ao0[r], 2e-2, "head outputs")
    _close(x1[r], want[r], 2e-2, "x1")
    # the typical element agrees far better than the worst one
    assert ((x1[r].float() - want[r].float()).abs().mean() <= 2e-3 * want[r].float().abs().mean()).item()
    assert ((qkv[r].float() - qkv0[r].float()).abs().mean() <= 1e-3 * qkv0[r].float().abs().mean()).item()
    if seq_off is None and rows == n_seq * S:
        # the decoder's per-sequence conditioning term in the same launch: x1 += drop(g[sequence]), one mask element per
        # (sequence, channel) - against dsvg_bcast_add_fwd on the unfused result
        g = (_rand(n_seq, 256, seed=41) * 0.7).to(torch.bfloat16)
        want_g = ops.bcast_add_fwd_(want.clone(), g, n_seq, S, p, 9, seed)
        x1g = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], km, n_seq, S, scale,
                                 1e-5, p, 7, 8, seed, train=False, seq_add=g, site_seq_add=9)
        _close(x1g, want_g, 2e-2, "x1 with the per-sequence add")
        assert not torch.equal(x1g, x1)
        # the same rows as a column block of a [n_seq, 1024] tensor (row stride 1024: how GlobalCondFn hands the rows of one
        # layer of a decoder stack over): bit-identical to the contiguous copy
        wide = (_rand(n_seq, 1024, seed=43) * 0.7).to(torch.bfloat16)
        wide[:, 512:768] = g
        x1s = ops.attn_block_fwd(x, packed, prm["in_bias"], prm["out_bias"], prm["gamma"], prm["beta"], km, n_seq, S, scale,
                                 1e-5, p, 7, 8, seed, train=False, seq_add=wide[:, 512:768], site_seq_add=9)
        assert wide[:, 512:768].stride(0) == 1024 and torch.equal(x1s, x1g), "strided conditioning rows"


def test_copy_many_and_bcast_add_bwd_tail(gpu_device):
    """dsvg_copy_many: 40 copies (two launches of the 32-entry table) of mixed dtypes, sizes from 1 element to several
    chunks, some of them at addresses that are not 16-byte aligned; dsvg_bcast_add_bwd with zero rows behind a live prefix"""
    g = torch.Generator(device="cpu").manual_seed(5)
    pairs, want = [], []
    for i in range(40):
        n = [1, 3, 7, 64, 1000, 4099, 70001, 300000][i % 8]
        dt = [torch.float32, torch.int32, torch.int64, torch.bfloat16, torch.uint8][i % 5]
        src = (torch.randn(n + 3, generator=g) * 100).to(DEV).to(dt)
        dst = torch.zeros(n + 3, dtype=dt, device=DEV)
        o = i % 3                                   # views that start 0, 1 or 2 elements into the buffer
        pairs.append((dst[o:o + n], src[o:o + n]))
        want.append((dst, src, o, n))
    ops.copy_many(pairs)
    torch.cuda.synchronize()
    for dst, src, o, n in want:
        assert torch.equal(dst[o:o + n], src[o:o + n])
        assert (dst[:o] == 0).all() and (dst[o + n:] == 0).all(), "wrote outside the destination range"
    dx = _rand(24 * 8, 256, dtype=torch.bfloat16, seed=9)
    seed = _seed_tensor(77)
    full = ops.bcast_add_bwd(dx, 24, 8, 0.1, 5, seed)
    part = ops.bcast_add_bwd(dx, 10, 8, 0.1, 5, seed, n_seq_out=24)
    assert torch.equal(part[:10], full[:10]) and (part[10:] == 0).all() and tuple(part.shape) == (24, 256)
    _close(full, R.bcast_add_bwd(dx, 24, 8, 0.1, 5, seed), 1e-2, "bcast_add_bwd")


def test_grouped_weight_gradient_launch_is_bit_identical(gpu_device):
    """ops.GROUP: the split-K weight-gradient GEMMs of a group-stage layer (4096 tokens; in_proj, out_proj, linear1, linear2
    and the 512-row conditioning projection) queued and run as one launch - with the reductions deferred (one launch for the
    GEMMs, one for the reductions) and with immediate reductions (each reduction first flushes the queued producers) - must
    reproduce the separate launches bit for bit, bias gradients (fused row sums) included"""
    T = 4096
    shapes = [(768, 256, T), (256, 256, T), (512, 256, T), (256, 512, T), (256, 256, 512)]
    ops_in = [(_rand(k, n_out, dtype=torch.bfloat16, seed=700 + i), _rand(k, k_in, dtype=torch.bfloat16, seed=710 + i))
              for i, (n_out, k_in, k) in enumerate(shapes)]

    def run(group, defer):
        outs = []
        ctxs = ([ops.DEFER] if defer else []) + ([ops.GROUP] if group else [])
        import contextlib
        with contextlib.ExitStack() as st:
            for c in ctxs:
                st.enter_context(c)
            for (dy, x), (n_out, k_in, k) in zip(ops_in, shapes):
                flat = torch.empty(n_out * k_in + n_out, device=DEV, dtype=torch.float32)
                dw, db = flat[:n_out * k_in].view(n_out, k_in), flat[n_out * k_in:]
                ops.gemm(dy, x, a_kc=False, b_kc=False, out=dw, split_k=ops.split_k_for(n_out, k_in, k), rowsum=db)
                outs.append(flat)
        ops.flush_deferred()
        torch.cuda.synchronize()
        return outs
    want = run(False, False)
    for group, defer in ((True, True), (True, False), (False, True)):
        got = run(group, defer)
        for i, (a, b) in enumerate(zip(got, want)):
            if defer:       # the deferred reduction sums the slices in another (fixed) order
                _close(a, b, 2e-6, f"grouped={group} deferred: problem {i}")
            else:
                assert torch.equal(a, b), f"grouped={group} immediate reductions: problem {i}"
    a, b = run(True, True), run(False, True)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"grouped vs separate launches (both deferred): problem {i}"


def test_loss_combine(gpu_device):
    scs = [torch.tensor([3.5, 7.0], device=DEV), torch.tensor([10.0, 4.0], device=DEV), torch.tensor([1.0, 8.0], device=DEV)]
    w = (1.0, 2.0, 0.5)
    out = ops.loss_combine_fwd(scs, w)
    want = R.loss_combine_fwd(scs, w)
    assert torch.allclose(out, want, rtol=1e-6, atol=0) and out.numel() == 4
    dt, d1 = torch.tensor([0.25], device=DEV), torch.tensor([3.0], device=DEV)
    got = ops.loss_combine_bwd(dt, [None, d1, None], w, torch.device(DEV))
    assert torch.allclose(got, R.loss_combine_bwd(dt, [None, d1, None], w, torch.device(DEV))) and tuple(got.shape) == (3, 2)
    assert torch.equal(ops.loss_combine_bwd(None, [None] * 3, w, torch.device(DEV)), torch.zeros(3, 2, device=DEV))


@pytest.mark.parametrize("packed", [False, True])
def test_masked_mean_bf16_is_the_sequential_fp32_sum(gpu_device, packed):
    """round 6: the bf16 forward pooling kernel reads 16 bytes per thread (a thread = 8 columns of one sequence); every column is
    still summed over its valid rows in increasing order in fp32, scaled by 1 / count and rounded once - EXACTLY this restatement,
    on both layouts (key masks / packed valid tokens); the backward pass: the scaled gradient row on the valid rows, zeros elsewhere
    (incl. the bucket tail of the packed layout)."""
    n_seq, S, d = 517, 32, 256
    g = torch.Generator(device="cpu").manual_seed(9)
    lens = torch.randint(1, S + 1, (n_seq,), generator=g)
    if packed:
        off = torch.zeros(n_seq + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(lens, 0).to(torch.int32)
        total = int(off[-1])
        rows = (total + 127) // 128 * 128 + 256
        x = _rand(rows, d, dtype=torch.bfloat16, seed=1)
        m = ops.masked_mean_fwd(x, None, n_seq, S, seq_off=off.to(DEV))
        row0 = off[:-1].long()
        bits = (torch.arange(S)[None, :] < lens[:, None])
    else:
        bits = torch.rand(n_seq, S, generator=g) < 0.6
        bits[torch.arange(n_seq), torch.randint(0, S, (n_seq,), generator=g)] = True
        km = (bits.to(torch.int64) << torch.arange(S, dtype=torch.int64)).sum(1).to(DEV)
        x = _rand(n_seq * S, d, dtype=torch.bfloat16, seed=1)
        m = ops.masked_mean_fwd(x, km, n_seq, S)
        row0 = torch.arange(n_seq) * S
    xf = x.float().cpu()
    acc = torch.zeros(n_seq, d)
    for i in range(S):
        idx = (row0 + i).clamp(max=xf.shape[0] - 1)
        acc = torch.where(bits[:, i:i + 1], acc + xf[idx], acc)
    inv = (1.0 / bits.sum(1).float())[:, None]          # (the kernel multiplies by the fp32 reciprocal of the count)
    want = (acc * inv).to(torch.bfloat16)
    assert torch.equal(m.cpu(), want)
    dm = _rand(n_seq, d, dtype=torch.bfloat16, seed=2)
    gv = (dm.float().cpu() * inv).to(torch.bfloat16)
    if packed:
        dx = ops.masked_mean_bwd(dm, None, n_seq, S, seq_off=off.to(DEV), total_rows=rows).cpu()
        exp = torch.zeros(rows, d, dtype=torch.bfloat16)
        for b in range(n_seq):
            exp[int(off[b]):int(off[b + 1])] = gv[b]
    else:
        dx = ops.masked_mean_bwd(dm, km, n_seq, S).cpu()
        exp = torch.where(bits.reshape(-1, 1), gv.repeat_interleave(S, 0), torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(dx, exp)
