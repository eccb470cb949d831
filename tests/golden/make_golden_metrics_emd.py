"""Generates tests/golden/metrics/metrics_emd.npz: the REAL reference's `svg_emd_loss`, `svg_length_loss` and
`continuity_loss` (deepsvg/difflib/loss.py:10-51) on clouds of its own `SVGTensor.sample_points`
(deepsvg/difflib/tensor.py:191-230), imported read-only from /root/reference.  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics_emd.py

Inputs: the short sequences of metrics_points.npz (lens <= 16), cut to 16 rows, in the five (pred, target) pairs PAIRS,
n = 4 samples per command (clouds of 4-31 points: on the n = 10 clouds of that fixture the arc-length match is within
3e-7 relative of a tie, which the reference's fp32 cumsum decides by chance).  The integer arguments are jittered as in
make_golden_metrics_grad.py (a seeded uniform +-0.185 in every slot of the whole args tensor).

The reference is run on DETACHED inputs: with the installed torch its `np.argmin` over a list of tensors
(loss.py:39) raises "Can't call numpy() on Tensor that requires grad" under autograd.  Recorded per pair, with
`first_point_weight` off and on: the reference's loss, and its matched indices (`return_matched_indices=True`) mapped from
its re-oriented target back to the target as passed (through its own `is_clockwise`).  The recorded GRADIENT is therefore
not the reference's backward of svg_emd_loss but torch autograd of what that function computes once the indices are
fixed: `norm(p_pred - p_target[matched], dim=-1)` (times the weights where the weight is on), `.mean()`, back through the
reference's own `sample_points` to the pred's args - the indices are the reference's own.

The generator asserts, on the float64 restatement (tests/emd_ref.py), and tries the next seed otherwise:
  the gap between the best and the second-best shift sum >= 1e-3 (as means, S / n); the gap between the nearest and the
  second-nearest arc-length match >= 1e-4; |A| >= 1; every matched pair's distance at the chosen shift >= 1e-2; no NaN;
  both orientations of the target occur.  All pairs must pass.

What is stored (float32 unless said):
  seed, pairs [5, 2] int32        the jitter seed in use, the (pred, target) sequences of metrics_points.npz
  commands_x, commands_y [5, 16]  args_x, args_y [5, 16, 11]: the jittered inputs
  loss, loss_w [5] float64        the reference's loss without / with first_point_weight
  matched [5, 49] int32           the reference's matched indices into the target as passed, -1 past the pred count
  shift [5] int32                 the float64 restatement's shift (its matched indices equal the reference's)
  flip [5] bool                   the reference re-oriented the target
  grad, grad_w [5, 16, 11] float64   the gradient described above, d / d args_x
  length_loss, continuity [5] float64   svg_length_loss(pred, target), continuity_loss(pred)
  ref_spread, loss_spread float64   the largest |recorded gradient - the float64 restatement's| and the same for the loss
                                  (both weights): what the reference's fp32 sampling and sums cost
  shift_gap, match_gap, min_area, min_dist float64   the four margins as measured
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

from deepsvg.difflib.loss import continuity_loss, svg_emd_loss, svg_length_loss     # noqa: E402
from deepsvg.difflib.tensor import SVGTensor                                        # noqa: E402
from deepsvg.difflib.utils import is_clockwise                                      # noqa: E402
from tests import emd_ref as ER                                                     # noqa: E402
from tests import metrics_grad_ref as GR                                            # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics")
JITTER = 0.185
N = 4
L = 16
PAIRS = [(0, 1), (1, 2), (5, 9), (2, 5), (9, 0)]
MIN_SHIFT_GAP, MIN_MATCH_GAP, MIN_AREA, MIN_DIST = 1e-3, 1e-4, 1.0, 1e-2


def reference(commands, args, lens):
    P = len(PAIRS)
    rec = {"loss": torch.zeros(P, dtype=torch.float64), "loss_w": torch.zeros(P, dtype=torch.float64),
           "grad": torch.zeros(P, L, 11, dtype=torch.float64), "grad_w": torch.zeros(P, L, 11, dtype=torch.float64),
           "flip": torch.zeros(P, dtype=torch.bool), "length_loss": torch.zeros(P, dtype=torch.float64),
           "continuity": torch.zeros(P, dtype=torch.float64)}
    matched = []
    for p, (i, j) in enumerate(PAIRS):
        li, lj = int(lens[i]), int(lens[j])
        leaf = args[i, :li].clone().requires_grad_(True)
        pred = SVGTensor.from_cmd_args(commands[i, :li], leaf).sample_points(N)
        with torch.no_grad():
            target = SVGTensor.from_cmd_args(commands[j, :lj], args[j, :lj]).sample_points(N)
        m = target.shape[0]
        flip = not bool(is_clockwise(target))
        rec["flip"][p] = flip
        rec["length_loss"][p] = float(svg_length_loss(pred.detach(), target))
        rec["continuity"][p] = float(continuity_loss(pred.detach()))
        for weighted, kl, kg in ((False, "loss", "grad"), (True, "loss_w", "grad_w")):
            loss, (_, oriented, idx) = svg_emd_loss(pred.detach(), target, first_point_weight=weighted,
                                                    return_matched_indices=True)
            rec[kl][p] = float(loss)
            terms = torch.norm(pred - oriented[idx], dim=-1)
            if weighted:
                w = torch.ones_like(terms)
                w[0] = 10.
                terms = terms * w
            g, = torch.autograd.grad(terms.mean(), leaf, retain_graph=True)
            rec[kg][p, :li] = g.double()
            as_passed = (m - 1 - idx) if flip else idx
            if weighted:
                assert torch.equal(as_passed, matched[-1]), "the weight moved the reference's matching"
            else:
                matched.append(as_passed)
    return rec, matched


def restated(commands, args):
    """-> loss, loss_w, grad, grad_w, shift, matched, margins: tests/emd_ref.py on float64 points"""
    i, j = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    cx, ax, cy, ay = commands[i, :L], args[i, :L], commands[j, :L], args[j, :L]
    px, nx = GR.sample_points64(cx, ax, N)
    py, ny = GR.sample_points64(cy, ay, N)
    res = {}
    for weighted, sfx in ((False, ""), (True, "_w")):
        out, shift, matched, t = ER.emd(px, nx, py, ny, weighted, as_double=True)
        dpx = ER.emd_bwd(px, nx, ny, t, shift, torch.ones(len(PAIRS), dtype=torch.float64), weighted, as_double=True)
        res["loss" + sfx], res["grad" + sfx] = out, GR.sample_points_bwd(cx, dpx, N, as_double=True)
    shift_gap = match_gap = area = dist = float("inf")
    for b in range(len(PAIRS)):
        n, m = int(nx[b]), int(ny[b])
        _, _, gap, A = ER.emd_match(n, py[b, :m])
        S = ER.shift_sums(px[b, :n], t[b, :n]) / n
        two = S.topk(2, largest=False).values
        s = int(shift[b])
        pair = (px[b, :n] - torch.cat([t[b, s:n], t[b, :s]])).norm(dim=-1)
        shift_gap, match_gap = min(shift_gap, float(two[1] - two[0])), min(match_gap, gap)
        area, dist = min(area, abs(A)), min(dist, float(pair.min()))
    return res, shift, matched, nx, (shift_gap, match_gap, area, dist)


def main():
    base = dict(np.load(os.path.join(OUT, "metrics_points.npz"), allow_pickle=False))
    commands, args0, lens = torch.from_numpy(base["commands"]), torch.from_numpy(base["args"]), base["lens"]
    assert all(int(lens[s]) <= L for p in PAIRS for s in p)
    for seed in range(1, 50):
        jit = (torch.rand(args0.shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * JITTER
        args = (args0 + jit).float()
        rec, ref_matched = reference(commands, args, lens)
        res, shift, matched, nx, (shift_gap, match_gap, area, dist) = restated(commands, args)
        finite = all(bool(torch.isfinite(v.double()).all()) for v in rec.values())
        same = all(torch.equal(ref_matched[b].to(torch.int32), matched[b, :int(nx[b])]) for b in range(len(PAIRS)))
        both = bool(rec["flip"].any()) and not bool(rec["flip"].all())
        ok = (shift_gap >= MIN_SHIFT_GAP and match_gap >= MIN_MATCH_GAP and area >= MIN_AREA and dist >= MIN_DIST and finite
              and same and both)
        print(f"seed {seed}: shift gap {shift_gap:.3e}, match gap {match_gap:.3e}, |A| {area:.3e}, pair distance {dist:.3e}, "
              f"finite {finite}, matched equal {same}, both orientations {both}: {'ok' if ok else 'skipped'}")
        if ok:
            break
    else:
        raise SystemExit("no seed passed")
    ref_spread = max((rec[k] - res[k]).abs().max().item() for k in ("grad", "grad_w"))
    loss_spread = max((rec[k] - res[k]).abs().max().item() for k in ("loss", "loss_w"))
    assert loss_spread < 1e-4
    i, j = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    out = {"seed": np.int32(seed), "pairs": np.asarray(PAIRS, dtype=np.int32),
           "commands_x": commands[i, :L].numpy(), "args_x": args[i, :L].numpy(),
           "commands_y": commands[j, :L].numpy(), "args_y": args[j, :L].numpy(),
           "matched": matched.numpy(), "shift": shift.numpy(), "flip": rec["flip"].numpy(),
           "ref_spread": np.float64(ref_spread), "loss_spread": np.float64(loss_spread),
           "shift_gap": np.float64(shift_gap), "match_gap": np.float64(match_gap), "min_area": np.float64(area),
           "min_dist": np.float64(dist)}
    out.update({k: rec[k].numpy() for k in ("loss", "loss_w", "grad", "grad_w", "length_loss", "continuity")})
    path = os.path.join(OUT, "metrics_emd.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; ref_spread {ref_spread:.3e}, loss_spread {loss_spread:.3e}, loss "
          f"{rec['loss'].tolist()}, weighted {rec['loss_w'].tolist()}, flip {rec['flip'].tolist()}, shift {shift.tolist()}, "
          f"counts {nx.tolist()}")


if __name__ == "__main__":
    main()
