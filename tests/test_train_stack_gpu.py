"""Train-mode gradients of the stacks and the dropout front ends on the device: the cases of tests/train_stack_ref.py through
the HIP kernels, against float64 autograd over the straight-line reference with the same dropout masks.

  fp32    relative L2 to the reference <= 1e-3 per tensor (forward output, dx, dz / dl, every parameter gradient).
  bf16    relative L2 to the reference <= 3 x d_round(tensor) per tensor.  d_round is computed here, on the CPU, by the same
          case through the restatements of tests/torch_ops_ref.py (same weights, inputs and seed): the rounding floor of the
          computation restated with storage rounding.  The factor 3 allows for accumulation order and the few points where a
          fused kernel rounds differently from the restatement; the bound never comes from the kernels' own output.  That 3 x
          d_round separates "right masks" from "one mask wrong" is what tests/test_train_stack_host.py guards, site by site.
  d_round itself is capped here from the reference alone, with one more reference pass in which EVERY site draws from another
          site: a tensor that pass moves must be moved by at least 2 x 3 x d_round(tensor).  The restated run goes through the
          same host logic as the kernels, so a wrong mask in an arm only a bf16 run takes (mask_site=, the fused and
          group-stage backward) would otherwise raise d_round and the bound with it.  Measured on the restatements: the pass
          moves the tensors with the largest d_round (4.5 - 6.5 %: ReLU gates that flip under bf16 rounding of their input) by
          70 - 90 %, a single wrong mask moves what lies behind it by 25 - 50 %.  The case of 16.4 k rows leaves this pass to
          the host file's site-by-site guard.
  route   the launches the case names ran (ffn_gate_dw2, the `masked=` arm of layernorm_bwd, ...).
  zeros   the inert packed rows' dx, the gradient rows of the sequences past a live prefix, the position-table rows past S:
          exactly zero.
Each case prints one line and, with DSVG_PARITY_LOG_DIR set, appends it to train_stack_parity.log in that directory (a run
of the final tree is committed as profiles/train_stack_parity.log)."""
import pytest

from tests import train_stack_ref as T

pytestmark = pytest.mark.gpu
LOG = "train_stack_parity.log"


ALL_WRONG_MAX_ROWS = 8192


def _compare(case, got, ref, emu, ref_all=None):
    d = T.distances(case, got, ref)
    if case.dtype == "fp32":
        d_round = None
        ratio = {k: v / T.FP32_BOUND for k, v in d.items()}
    else:
        d_round = T.distances(case, emu, ref)
        ratio = {k: v / max(T.BF16_FACTOR * d_round[k], 1e-30) for k, v in d.items()}
    for k in sorted(d, key=lambda k_: -ratio[k_]):          # every figure before any assertion
        print(f"   {case.id} {k}: error {d[k]:.3e}" + (f", d_round {d_round[k]:.3e}, error / d_round {d[k] / max(d_round[k], 1e-30):.2f}"
                                                      if d_round is not None else ""))
    worst = max(ratio, key=ratio.get)
    if d_round is None:
        line = f"{case.id}: worst {worst} error {d[worst]:.3e} (bound 1e-3), forward {d['out']:.3e}"
    else:
        line = (f"{case.id}: worst {worst} error {d[worst]:.3e}, d_round {d_round[worst]:.3e}, ratio "
                f"{d[worst] / max(d_round[worst], 1e-30):.2f} (bound {T.BF16_FACTOR:g}), forward {d['out']:.3e} / {d_round['out']:.3e}")
    T.parity_log(LOG, line)
    if ref_all is not None:
        moved = T.distances(case, ref_all, ref)
        for k, m in moved.items():
            if m >= 1e-9:           # (the final LayerNorm's bias gradient is the column sum of dout: no site moves it)
                assert d_round[k] <= m / (2 * T.BF16_FACTOR), \
                    (case.id, f"{k}: the restated bf16 run is off the reference by {d_round[k]:.3e}; every mask wrong moves it by {m:.3f}")
    assert ratio["out"] <= 1.0, (case.id, "forward", d["out"])
    assert ratio[worst] <= 1.0, (case.id, worst, d[worst], None if d_round is None else d_round[worst])
    for what, t in T.exact_zeros(case, got):
        assert t.numel() > 0 and not bool(t.any()), (case.id, what)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_stack_gradients_match_autograd(case, gpu_device, monkeypatch):
    got, params, inp = T.run_stack_case(case, gpu_device, monkeypatch, on_gpu=True)
    ref = T.reference_for(case, params, inp)
    emu = ref_all = None
    if case.dtype == "bf16":
        with T.emulated(long_paths=case.kind == "long126"):
            emu = T.run_stack_case(case, "cpu", monkeypatch)[0]
        if case.rows <= ALL_WRONG_MAX_ROWS:
            ref_all = T.reference_for(case, params, inp, wrong_site="all")
    _compare(case, got, ref, emu, ref_all)


@pytest.mark.parametrize("case", T.FRONT_CASES, ids=lambda c: c.id)
def test_front_end_gradients_match_autograd(case, gpu_device, monkeypatch):
    got, params, inp = T.run_front_case(case, gpu_device, monkeypatch, on_gpu=True)
    ref = T.front_reference(case, params, inp, T.seed_tensor())
    emu = ref_all = None
    if case.dtype == "bf16":
        with T.emulated():
            emu = T.run_front_case(case, "cpu", monkeypatch)[0]
        ref_all = T.front_reference(case, params, inp, T.seed_tensor(), wrong_site=case.site)
    _compare(case, got, ref, emu, ref_all)
