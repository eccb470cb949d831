"""Train-mode wiring of the stacks and the dropout front ends on the CPU: every case of tests/train_stack_ref.py through the
product with the restatements of tests/torch_ops_ref.py in place of `ops`, against float64 autograd over the straight-line
reference with the same dropout masks.

  fp32   every compared tensor within 1e-3 relative L2 of the reference.
  bf16   this run DEFINES d_round(tensor): the distance of the restated bf16 computation (storage rounding, fp32 sums) to the
         float64 reference on the same bf16 weights and inputs.  tests/test_train_stack_gpu.py bounds the kernels by
         3 x d_round.  Nothing bounds d_round itself but the guard below.
  guard  from the reference alone: moving ONE site's mask to another site (wrong_site=) must move some compared tensor by at
         least twice its bound (1e-3, or 3 x d_round) - for every site of every case - and every compared tensor that depends
         on a mask must be moved that far by the site that moves it most.  A case whose bound could not tell "right masks" from
         "one mask wrong" fails here; so does a bf16 run whose distance to the reference is a wrong mask's, not rounding's.
The forward comparison comes first: a mis-indexed mask is a 5-10 % forward error."""
import pytest

from tests import long_ops_ref as LR
from tests import train_stack_ref as T

# forward output of a bf16 run: activation rounding only (2^-9 per stored value, a handful of stores per layer) - a mask on
# the wrong rows moves it by 5-10 %, so 2 % separates the two whatever the guard says about the gradients
BF16_FORWARD_BOUND = 2e-2


def _bound(case, name, d_round):
    return T.FP32_BOUND if case.dtype == "fp32" else T.BF16_FACTOR * d_round[name]


def _check_case(case, got, ref, refs_wrong):
    d = T.distances(case, got, ref)
    print(f"{case.id}: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(d.items(), key=lambda kv: -kv[1])[:6]))
    assert d["out"] <= (T.FP32_BOUND if case.dtype == "fp32" else BF16_FORWARD_BOUND), (case.id, "forward", d["out"])
    if case.dtype == "fp32":
        worst = max(d, key=d.get)
        assert d[worst] <= T.FP32_BOUND, (case.id, worst, d[worst])
    for what, t in T.exact_zeros(case, got):
        assert t.numel() > 0 and not bool(t.any()), (case.id, what)
    # the guard: every site has a witness
    dws = {site: T.distances(case, wrong, ref) for site, wrong in refs_wrong.items()}
    for site, dw in dws.items():
        margin = {k: dw[k] / max(2 * _bound(case, k, d), 1e-30) for k in dw}
        best = max(margin, key=margin.get)
        print(f"   site {site}: witness {best} moves {dw[best]:.3f} = {margin[best]:.2f} x (2 x bound {_bound(case, best, d):.2e})")
        assert margin[best] >= 1.0, (case.id, f"no witness for site {site}", best, dw[best], _bound(case, best, d))
    # ... and every tensor is a witness of the site that moves it most.  This is what bounds d_round: a wrong mask in an arm only
    # a bf16 run takes (mask_site=, the fused and group-stage backward) inflates d_round of the tensors behind it to the size of
    # a wrong-site shift, which the site-by-site guard above does not notice as long as ANOTHER tensor still witnesses the site.
    # (Exempt: a tensor no site moves at all - the final LayerNorm's bias gradient is the column sum of dout.)
    moved = {k: max(dw[k] for dw in dws.values()) for k in d}
    for k, m in sorted(moved.items(), key=lambda kv: kv[1] / max(_bound(case, kv[0], d), 1e-30)):
        if m < 1e-9:
            continue
        assert m >= 2 * _bound(case, k, d), (case.id, f"{k}: off the reference by {d[k]:.3e}, so its bound {_bound(case, k, d):.3e} "
                                             f"cannot tell the shift {m:.3f} of its most influential site from rounding")


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_stack_gradients_match_autograd_with_emulated_ops(case, emulated_ops, monkeypatch):
    saved = LR.install() if case.kind == "long126" else None      # (the S > 64 restatements, on top of the fixture's)
    try:
        got, params, inp = T.run_stack_case(case, "cpu", monkeypatch)
    finally:
        if saved is not None:
            LR.restore(saved)
    ref = T.reference_for(case, params, inp)
    wrong = {s: T.reference_for(case, params, inp, wrong_site=s) for s in case.sites()}
    _check_case(case, got, ref, wrong)


@pytest.mark.parametrize("case", T.FRONT_CASES, ids=lambda c: c.id)
def test_front_end_gradients_match_autograd_with_emulated_ops(case, emulated_ops, monkeypatch):
    got, params, inp = T.run_front_case(case, "cpu", monkeypatch)
    ref = T.front_reference(case, params, inp, T.seed_tensor())
    wrong = {case.site: T.front_reference(case, params, inp, T.seed_tensor(), wrong_site=case.site)}
    _check_case(case, got, ref, wrong)
