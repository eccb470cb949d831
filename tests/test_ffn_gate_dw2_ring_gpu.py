"""The tile ring of ops.ffn_gate_dw2 (csrc/ffn_bwd_gate.hip) at its edges: slices of fewer tiles than the ring has slots, exactly
as many, one and two more, a last tile of one row, empty slices, a short last slice.  split_k = 8 is passed explicitly, so a slice
is ceil(T / 8) rows rounded up to 64 and the row counts below are the smallest that reach each case.  Reference: the two launches
the kernel replaces, on the same inputs."""
import functools

import pytest
import torch

DEV = "cuda"
SPLIT_K = 8
# 1 ... 6 tiles per slice; 2049: 320-row slices, slice 6 ends in a one-row tile, slice 7 is empty; 40: one ragged tile, seven empty
# slices; 4160: 576-row slices of nine tiles, the last slice short
ROWS = [512, 1024, 1536, 2048, 2560, 3072, 2049, 40, 4160]


def _inputs(T, drop, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dym = (torch.randn(T, 256, generator=g) * 0.5).to(DEV, torch.bfloat16)
    hp = torch.relu(torch.randn(T, 512, generator=g))
    if drop > 0:        # h > 0 <=> ReLU passed AND the hidden dropout kept it
        hp = hp * (torch.rand(T, 512, generator=g) >= drop)
    hp = hp.to(DEV, torch.bfloat16)
    w2p = (torch.randn(256, 512, generator=g) * 0.05).to(DEV, torch.bfloat16)
    return dym, hp, w2p


@functools.lru_cache(maxsize=None)
def _case(T, drop):
    """inputs, gate scale and the two launches' results for (T, drop): computed once, shared, never written to"""
    from deepsvg_amd import ops
    dym, hp, w2p = _inputs(T, drop, seed=1000 + T + int(drop * 10))
    scale = ops.keep_scale(drop)
    g2p = torch.empty((256, 512), dtype=torch.float32, device=DEV)
    db2 = torch.empty(256, dtype=torch.float32, device=DEV)
    ops.gemm(dym, hp, a_kc=False, b_kc=False, out=g2p, split_k=SPLIT_K, rowsum=db2)
    dpre = ops.gemm(dym, w2p, b_kc=False, gate=hp, gate_scale=scale)
    torch.cuda.synchronize()
    return dym, hp, w2p, scale, (dpre, g2p, db2)


def _nan_outputs():
    return (torch.full((256, 512), float("nan"), dtype=torch.float32, device=DEV),
            torch.full((256,), float("nan"), dtype=torch.float32, device=DEV))


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _check(T, got, ref):
    dpre, g2p, db2 = got
    assert torch.equal(dpre, ref[0]), "dpre differs from the gated GEMM"
    assert torch.isfinite(g2p).all() and torch.isfinite(db2).all(), "a NaN of the pre-filled outputs survived"
    if T % 64 == 0:
        assert torch.equal(g2p, ref[1]), "G2p differs from the split-K GEMM's"
        assert torch.equal(db2, ref[2]), "db2 differs from the split-K GEMM's"
    else:
        print(f"T={T}: rel L2 G2p {_rel_l2(g2p, ref[1]):.3e}, db2 {_rel_l2(db2, ref[2]):.3e}")
        assert _rel_l2(g2p, ref[1]) <= 1e-5, _rel_l2(g2p, ref[1])
        assert _rel_l2(db2, ref[2]) <= 1e-5, _rel_l2(db2, ref[2])


@pytest.mark.gpu
@pytest.mark.parametrize("T", ROWS)
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_ring_edges_match_the_two_launches(gpu_device, T, drop):
    from deepsvg_amd import ops
    dym, hp, w2p, scale, ref = _case(T, drop)
    runs = []
    for _ in range(2):
        g2p, db2 = _nan_outputs()
        dpre = ops.ffn_gate_dw2(dym, hp, w2p, scale, g2p, db2, SPLIT_K)
        runs.append((dpre, g2p, db2))
    torch.cuda.synchronize()
    _check(T, runs[0], ref)
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two launches on the same inputs differ"


@pytest.mark.gpu
def test_ring_edges_inside_a_deferral_scope(gpu_device):
    """five tiles per slice (one more than the deepest ring has slots), G2p / db2 queued: valid after flush_deferred.  The queued
    reduction adds the slices in another order than the immediate one, so the split-K GEMM is queued in the same scope"""
    from deepsvg_amd import ops
    T = 2560
    dym, hp, w2p, scale, ref = _case(T, 0.1)
    g2p, db2 = _nan_outputs()
    ref_g2p, ref_db2 = _nan_outputs()
    with ops.DEFER:
        dpre = ops.ffn_gate_dw2(dym, hp, w2p, scale, g2p, db2, SPLIT_K)
        ops.gemm(dym, hp, a_kc=False, b_kc=False, out=ref_g2p, split_k=SPLIT_K, rowsum=ref_db2)
    ops.flush_deferred()
    torch.cuda.synchronize()
    _check(T, (dpre, g2p, db2), (ref[0], ref_g2p, ref_db2))
    assert _rel_l2(g2p, ref[1]) <= 1e-5 and _rel_l2(db2, ref[2]) <= 1e-5


@pytest.mark.gpu
def test_rows_past_the_end_of_dpre_stay_untouched(gpu_device):
    """the last tile of slice 6 holds one row and slice 7 none: nothing is stored at or past row T of an over-allocated dpre"""
    from deepsvg_amd import lib, ops
    T, T_alloc = 2049, 2049 + 192
    dym, hp, w2p, scale, ref = _case(T, 0.1)
    L = lib.load()
    sentinel = 0x7B7B       # a finite bf16 pattern that no product yields by chance in every element
    dpre = torch.full((T_alloc, 512), sentinel, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    g2p, db2 = _nan_outputs()
    ws = ops._ws(L.dsvg_gemm_workspace_bytes(256, 512, SPLIT_K), dym.device)
    lib.check(L.dsvg_ffn_gate_dw2(dym.data_ptr(), hp.data_ptr(), w2p.data_ptr(), float(scale), dpre.data_ptr(), T, SPLIT_K,
                                  g2p.data_ptr(), db2.data_ptr(), ws.data_ptr(), ws.numel() * 4, ops._stream()),
              "dsvg_ffn_gate_dw2")
    torch.cuda.synchronize()
    _check(T, (dpre[:T], g2p, db2), ref)
    assert bool((dpre[T:].view(torch.int16) == sentinel).all()), "rows past T of dpre were written"
