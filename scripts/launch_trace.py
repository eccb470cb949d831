"""Launch trace of one training step: every call of a public function of deepsvg_amd.ops, in order, with its scalar arguments
and the shape / strides / dtype of its tensor arguments (never an address).  Prints the number of records and a sha1 of the
list per set-up; --dump FILE writes the lists as text.  For comparing two trees (a refactor leaves the trace as it is, a
performance change shows which launches it moved): only deepsvg_amd and tests are imported, so the same file runs from a
checkout of another commit.  --cpu: the plain-torch restatements of the ops, six small set-ups; otherwise two bf16 steps of
the hierarchical_ordered model at 512 icons on the GPU, with the loss dict and a sha1 of the flat gradient buffer."""
import argparse
import functools
import hashlib
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepsvg_amd                                  # noqa: E402
from deepsvg_amd import ops, functional as Fn       # noqa: E402
from deepsvg_amd.synthetic import make_batch, make_batch_onestage, det_state_dict   # noqa: E402
from deepsvg_amd.trainer import TrainStep, DEFAULT_WEIGHTS                          # noqa: E402

TRACE = []
DEFAULTS = (Fn.FFN_MIN_ROWS, Fn.ATTN_MIN_ROWS, Fn.SEQ_ROUND, Fn.GS_REMAINDER)


def _desc(v):
    if torch.is_tensor(v):
        return f"T{tuple(v.shape)}{tuple(v.stride())}{str(v.dtype)[6:]}"
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(_desc(e) for e in v) + "]"
    if isinstance(v, dict):     # (keyed by anything but names - ParamStore's id(param) index: the size only)
        named = all(isinstance(k, str) for k in v)
        return "{" + ",".join(f"{k}:{_desc(e)}" for k, e in v.items()) + "}" if named else f"dict[{len(v)}]"
    return repr(v) if v is None or isinstance(v, (bool, int, float, str, torch.dtype)) else type(v).__name__


def install_recorder():
    for name, fn in list(vars(ops).items()):
        if not name.startswith("_") and isinstance(fn, types.FunctionType):
            def rec(*a, _f=fn, _n=name, **kw):
                TRACE.append(_n + "(" + ",".join([_desc(v) for v in a] + [f"{k}={_desc(v)}" for k, v in kw.items()]) + ")")
                return _f(*a, **kw)
            setattr(ops, name, functools.wraps(fn)(rec))


def report(tag, dump, extra):
    text = "\n".join(TRACE) + "\n"
    print(f"{tag}: {len(TRACE)} records, trace sha1 {hashlib.sha1(text.encode()).hexdigest()}{extra}", flush=True)
    if dump:
        with open(dump, "a") as f:
            f.write(f"==== {tag}\n{text}")


def cpu_setup(tag, kind, dtype, shrink, trainer, dump):
    from tests import helpers as H
    cfg = H.build_cfg(kind)
    cfg.n_layers = cfg.n_layers_decode = 2
    cfg.dropout = 0.1
    one = kind.startswith("onestage")
    c, a = make_batch_onestage(6, total_len=cfg.max_total_len, seed=21) if one else make_batch(6, seed=21)
    label = (torch.arange(6) % cfg.n_labels) if cfg.label_condition else None
    if shrink:      # the routes of the large stages and the remainder split, at 6 icons
        Fn.FFN_MIN_ROWS, Fn.ATTN_MIN_ROWS, Fn.SEQ_ROUND, Fn.GS_REMAINDER = 64, 64, 8, 7
    else:
        Fn.FFN_MIN_ROWS, Fn.ATTN_MIN_ROWS, Fn.SEQ_ROUND, Fn.GS_REMAINDER = DEFAULTS
    torch.manual_seed(3)
    model = deepsvg_amd.SVGTransformer(cfg).train()
    model.load_state_dict(H.weights_for(model, 10))
    model.set_compute_dtype(dtype)
    TRACE.clear()
    if trainer:     # rt.defer: queued reductions, one grouped weight-gradient launch per group-stage stack
        ld = TrainStep(model, deepsvg_amd.SVGLoss(cfg), lr=0.0, use_graph=False).step(c, a, label=label)
    else:
        ld = deepsvg_amd.SVGLoss(cfg)(model(c, a, c, a, label=label, params={}), label, weights=DEFAULT_WEIGHTS)
        ld["loss"].backward()
    report(tag, dump, f", loss {float(ld['loss'].detach()):.9g}")


def gpu_run(dump):
    dev = torch.device("cuda:0")
    cfg = deepsvg_amd.HierarchicalOrdered()
    cfg.dropout = 0.1
    torch.manual_seed(3)        # (the dropout seed of the first step is torch's initial seed)
    model = deepsvg_amd.SVGTransformer(cfg)
    model.load_state_dict(det_state_dict(model, seed=77))
    model.to(dev).set_compute_dtype(torch.bfloat16).train()
    ts = TrainStep(model, deepsvg_amd.SVGLoss(cfg).to(dev), lr=0.0, use_graph=False)
    c, a = (t.to(dev) for t in make_batch(512, seed=21))
    for k in range(2):
        TRACE.clear()
        ld = ts.step(c, a)
        torch.cuda.synchronize()
        g = model.store.grad_buffer(0).detach().cpu().contiguous().numpy().tobytes()
        report(f"gpu step {k}", dump, f"\n  loss {({n: float(v) for n, v in sorted(ld.items())})}\n"
                                      f"  grad sha1 {hashlib.sha1(g).hexdigest()}")


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--dump", metavar="FILE")
    args = ap.parse_args()
    if args.dump:
        open(args.dump, "w").close()
    if args.cpu:
        from tests.conftest import install_emulated_ops
        install_emulated_ops()
    install_recorder()
    if not args.cpu:
        return gpu_run(args.dump)
    bf = torch.bfloat16
    for setup in (("a hier", "hier", bf, False, False), ("b hier shrunk", "hier", bf, True, False),
                  ("c hier shrunk TrainStep", "hier", bf, True, True), ("d onestage shrunk", "onestage", bf, True, False),
                  ("e onestage_label shrunk", "onestage_label", bf, True, False), ("f hier fp32", "hier", torch.float32, False, False)):
        cpu_setup(*setup, args.dump)


if __name__ == "__main__":
    main()
