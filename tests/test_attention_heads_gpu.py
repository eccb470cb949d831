"""The attention kernels at head counts other than the model's 8 (csrc/attention.hip, attention_mfma.hip, long_seq.hip)
against the plain-torch restatement of tests/torch_ops_ref.py evaluated in float64 on the same inputs.

The launchers take the head count at run time: it decides the head group of a workgroup (DSVG_ATTN_DISPATCH), the grid's
second dimension (H / HG) and the dropout row index ((b * H + h) * Smax + i).  Which kernel a case runs:

    H   S    fp32 / causal bf16   bf16, not causal
    4   31   <32,2>               <32,2>   (dsvg_attention_mfma_ok wants H % 8 == 0: no MFMA at 4 heads)
    4   52   <64,4>               <64,4>
    2   20   <32,2>               <32,2>
    6   9    <32,2>               <32,2>
    12  40   <64,4>               <64,4>
    16  8    <8,8>, H / HG = 2    MFMA, several sequences per 32-row tile, two head groups
    16  32   <32,8>, H / HG = 2   MFMA, two head groups
    6   40   <64,1>               <64,1>   (neither 8 | H nor 4 | H: one head per workgroup)
    3   20   <64,1>               <64,1>   (odd head count: one head per workgroup at every length)
    3   40   <64,1>               <64,1>

Tolerances are those of test_attention, test_attention_causal, test_attention_packed_layout and test_attention_long
(tests/test_kernels_gpu.py) at 8 heads: the arithmetic of one head does not depend on how many there are."""
import pytest
import torch

from deepsvg_amd import ops
from tests import torch_ops_ref as R
from tests.test_kernels_gpu import DEV, DTYPES, _close, _key_masks, _packed_case, _rand, _seed_tensor

pytestmark = pytest.mark.gpu

SCALE = 32 ** -0.5
# (H, S, n_seq): n_seq between 5 and 9, never a multiple of what a tile or a workgroup holds
SHAPES = [(4, 31, 7), (4, 52, 5), (2, 20, 9), (6, 9, 7), (12, 40, 5), (16, 8, 9), (16, 32, 5), (6, 40, 6), (3, 20, 7),
          (3, 40, 5)]
DROPS = (0.0, 0.1)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_blocks():
    """tests that run later measure how much device memory an op allocates (tests/test_draw_grad_gpu.py and its kind): a
    free block this file leaves in torch's caching allocator would be handed to them whole, slack included"""
    yield
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["dense", "masked", "causal"])
@pytest.mark.parametrize("H,S,n_seq", SHAPES)
def test_attention_head_counts(gpu_device, dtype, layout, H, S, n_seq):
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=100 * H + S)
    do = _rand(n_seq * S, 32 * H, dtype=dtype, seed=100 * H + S + 1)
    km = _key_masks(n_seq, S, seed=100 * H + S + 2, all_valid=layout == "dense")
    causal = layout == "causal"
    if causal and n_seq % 2:        # causal with and without a key mask (valid prefixes: key 0 is always visible)
        km = None
    seed = _seed_tensor(0x0123456789ABCDEF)
    site = 21 if not causal else 23
    for p in DROPS:
        o = ops.attention_fwd(qkv, km, n_seq, S, H, SCALE, p, site, seed, causal=causal)
        orf = R.attention_fwd(qkv.double(), km, n_seq, S, H, SCALE, p, site, seed, causal=causal)
        assert orf.dtype == torch.float64
        _close(o, orf, 3e-6 if dtype == torch.float32 else 1.5e-2, f"attn fwd H={H} S={S} {layout} p={p}")
        dq = ops.attention_bwd(qkv, km, do, n_seq, S, H, SCALE, p, site, seed, causal=causal)
        dqr = R.attention_bwd(qkv.double(), km, do.double(), n_seq, S, H, SCALE, p, site, seed, causal=causal)
        _close(dq, dqr, 1e-5 if dtype == torch.float32 else 2e-2, f"attn bwd H={H} S={S} {layout} p={p}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,S,n_seq", [s for s in SHAPES if s[1] <= 32])
def test_attention_head_counts_packed_layout(gpu_device, dtype, H, S, n_seq):
    """variable-length sequences back to back (seq_off), with and without the tile list; pad rows stay zero"""
    d = 32 * H
    km, off, total = _packed_case(n_seq, S, 5 + H)
    rows = (total + 127) // 128 * 128
    qkv = _rand(rows, 3 * d, dtype=dtype, seed=50 + H)
    do = _rand(rows, d, dtype=dtype, seed=51 + H)
    seed = _seed_tensor(0x1111222233334444)
    tiles = ops.attention_tiles(off, n_seq, 32)
    ref_t = R.attention_tiles(off, n_seq, 32)
    n_tiles = int(ref_t[n_seq + 1])
    assert int(tiles[n_seq + 1]) == n_tiles and torch.equal(tiles[:n_tiles + 1], ref_t[:n_tiles + 1])
    for p in DROPS:
        ref = R.attention_fwd(qkv.double(), None, n_seq, S, H, SCALE, p, 17, seed, seq_off=off)
        dref = R.attention_bwd(qkv.double(), None, do.double(), n_seq, S, H, SCALE, p, 17, seed, seq_off=off)
        for t in (None, tiles):
            what = f"H={H} S={S} p={p} {'tiled' if t is not None else 'untiled'}"
            out = ops.attention_fwd(qkv, None, n_seq, S, H, SCALE, p, 17, seed, seq_off=off, tiles=t)
            _close(out, ref, 2e-5 if dtype == torch.float32 else 2e-2, f"packed attention fwd {what}")
            assert torch.count_nonzero(out[total:]) == 0
            dq = ops.attention_bwd(qkv, None, do, n_seq, S, H, SCALE, p, 17, seed, seq_off=off, tiles=t)
            _close(dq, dref, 5e-5 if dtype == torch.float32 else 3e-2, f"packed attention bwd {what}")
            assert torch.count_nonzero(dq[total:]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,S,n_seq,masked,causal", [(4, 65, 5, True, False), (16, 130, 5, False, True)])
def test_attention_long_head_counts(gpu_device, dtype, H, S, n_seq, masked, causal):
    """sequences of more than 64 tokens (csrc/long_seq.hip): one workgroup per (sequence, head)"""
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=S + 60)
    do = _rand(n_seq * S, 32 * H, dtype=dtype, seed=S + 61)
    lens = None
    if masked:
        g = torch.Generator().manual_seed(S)
        lens = torch.randint(1, S + 1, (n_seq,), generator=g).to(torch.int32)
        lens[0], lens[-1] = S, 1
        lens = lens.to(DEV)
    seed = _seed_tensor(0x13572468ACE02468)
    for p in DROPS:
        o = ops.attention_fwd(qkv, lens, n_seq, S, H, SCALE, p, 29, seed, causal=causal)
        orf = R.attention_fwd(qkv.double(), lens, n_seq, S, H, SCALE, p, 29, seed, causal=causal)
        _close(o, orf, 5e-6 if dtype == torch.float32 else 1.5e-2, f"long attn fwd H={H} S={S} p={p}")
        dq = ops.attention_bwd(qkv, lens, do, n_seq, S, H, SCALE, p, 29, seed, causal=causal)
        dqr = R.attention_bwd(qkv.double(), lens, do.double(), n_seq, S, H, SCALE, p, 29, seed, causal=causal)
        _close(dq, dqr, 2e-5 if dtype == torch.float32 else 2e-2, f"long attn bwd H={H} S={S} p={p}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,S", [(6, 40), (3, 20), (3, 40)])
def test_attention_one_head_per_workgroup_refusal_leaves_the_output_alone(gpu_device, dtype, H, S):
    """H = 6 at 33..64 tokens and H = 3 at any length have a kernel (the <64,1> instantiation; the cases above compare it
    with the reference).  What the library does refuse at these shapes - dropout without a seed - it refuses before any
    launch: its own error, and the output buffer, pre-filled with a sentinel, is untouched"""
    from deepsvg_amd.lib import DsvgError
    n_seq = 5
    qkv = _rand(n_seq * S, 3 * 32 * H, dtype=dtype, seed=1)
    out = torch.full((n_seq * S, 32 * H), 7.0, dtype=dtype, device=DEV)
    with pytest.raises(DsvgError, match="dropout needs a seed"):
        ops.attention_fwd(qkv, None, n_seq, S, H, SCALE, 0.1, 21, None, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ops.attention_fwd(qkv, None, n_seq, S, H, SCALE, out=out)          # ... and the same call without dropout runs
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
