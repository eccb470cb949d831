"""Poisoned uninitialised memory: a context manager under which every `torch.empty` / `torch.empty_like` comes back filled.

The product allocates every workspace and output with those two constructors and clears none of them; whatever a kernel
reads from one before writing it is whatever the caching allocator left there.  Two runs of the same code, one with every
floating buffer born as NaN and one with it born as 0.0, must give bit-identical results: a difference is a read of memory
nobody wrote.

Integer and bool buffers are zero-filled in BOTH runs: a stale index must never become an out-of-range address because of a
test (that would provoke a fault, not detect a dependence).

Narrowing a failure: pass `log=[]` to collect the (file, line) of every allocation site inside deepsvg_amd/ (in order of first
use, no duplicates), then pass halves of that list as `only=` until one site is left."""
import contextlib
import os
import sys

import torch

PRODUCT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepsvg_amd") + os.sep


def _site():
    """(file relative to the repository, line) of the innermost frame inside deepsvg_amd/ that led to the allocation, or None"""
    f = sys._getframe(2)
    while f is not None:
        name = f.f_code.co_filename
        if name.startswith(PRODUCT_DIR):
            return ("deepsvg_amd/" + name[len(PRODUCT_DIR):].replace(os.sep, "/"), f.f_lineno)
        f = f.f_back
    return None


@contextlib.contextmanager
def poisoned_empty(float_fill, *, only=None, log=None):
    """float_fill: value of every floating (and complex) element; integer / bool elements are 0 whatever it is.
    only: iterable of (file, line) sites - poison those allocations only (the others stay uninitialised).
    log: list that receives the (file, line) of each allocation site inside deepsvg_amd/ once."""
    only = None if only is None else {(str(f), int(l)) for f, l in only}
    seen = set(log) if log is not None else None
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def fill(t):
        if only is not None or log is not None:
            site = _site()
            if log is not None and site is not None and site not in seen:
                seen.add(site)
                log.append(site)
            if only is not None and site not in only:
                return t
        with torch.no_grad():
            if t.is_floating_point() or t.is_complex():
                t.fill_(float_fill)
            else:
                t.zero_()
        return t

    def empty(*args, **kwargs):
        return fill(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return fill(real_empty_like(*args, **kwargs))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


def three_runs(fn):
    """fn() clean, under NaN poison and under zero poison -> the three results"""
    out = [fn()]
    for v in (float("nan"), 0.0):
        with poisoned_empty(v):
            out.append(fn())
    return out
