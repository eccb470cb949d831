"""Generates tests/golden/paths/filling.npz by running the REAL reference walk, `SVGPathGroup.compute_filling`
(deepsvg/svglib/svg_primitive.py:392-420, imported read-only from the reference checkout: DEEPSVG_REFERENCE, default
/root/reference), on real `SVGPath` squares of chosen orientation with `overlap_graph` patched to return an `nx.DiGraph` of a
given adjacency - the reference's own overlap measure needs shapely, which is not installed here, and the overlap measure of
this package is its own anyway (include/dsvg.h).  Run in the build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_filling.py

networkx is the real one; the reference's drawing stack is stubbed with the stub list of make_golden_paths.py.  Two families
at G = 8: transitive closures of random forests under a random labelling (nested shapes), and random digraphs with edge
probability 0.15.  The reference iterates Python sets inside a level; a case is ORDER-FREE when the restatement
(tests/paths_fill_ref.filling_from_counts) gives the same result ascending and descending, and only those are compared.
Asserted here: every forest is order-free, at least 95 % of the random family is, and on every order-free case the reference
equals the restatement under rule="orientation".  Stored (data only): adjacency as one uint8 bit mask per source row
(bit i of adj[n, j] = an edge j -> i), clockwise bool [N, 8], family uint8 [N] (0 forest, 1 random), order_free bool [N],
filling int8 [N, 8] as the reference left it (0 where it never set one)."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("DEEPSVG_REFERENCE", "/root/reference"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


class _Stub:
    def __getattr__(self, k):
        return _Stub()

    def __call__(self, *a, **k):
        return _Stub()

    def __mro_entries__(self, bases):
        return (object,)


for _name in ["cairosvg", "IPython", "IPython.display", "moviepy", "moviepy.editor", "shapely", "shapely.geometry",
              "shapely.ops", "torchvision", "torchvision.utils", "torchvision.transforms",
              "torchvision.transforms.functional", "tensorboardX", "PIL", "PIL.Image", "PIL.ImageOps",
              "matplotlib", "matplotlib.pyplot", "matplotlib.figure", "matplotlib.colors"]:
    try:
        __import__(_name)
    except Exception:
        _m = types.ModuleType(_name)
        _m.__file__ = "/dev/null"
        _m.__getattr__ = lambda k: _Stub()
        sys.modules[_name] = _m

import networkx as nx                                             # noqa: E402  (the real one)
from deepsvg.svglib.geom import Point                             # noqa: E402
from deepsvg.svglib.svg_command import SVGCommandLine             # noqa: E402
from deepsvg.svglib.svg_path import SVGPath                       # noqa: E402
from deepsvg.svglib.svg_primitive import SVGPathGroup             # noqa: E402
from tests import paths_fill_ref as FR                            # noqa: E402

G = 8
OUT = os.path.join(HERE, "paths")


def square_path(clockwise):
    """a closed SVGPath square whose is_clockwise() is `clockwise`"""
    corners = [(10., 10.), (50., 10.), (50., 50.), (10., 50.)]
    if not clockwise:
        corners = corners[::-1]
    pts = [Point(*c) for c in corners]
    path = SVGPath([SVGCommandLine(pts[i], pts[(i + 1) % 4]) for i in range(4)], closed=True)
    if path.is_clockwise() != clockwise:
        path = path.reverse()
    assert path.is_clockwise() == clockwise
    return path


def reference(adj, cw):
    graph = nx.DiGraph()
    graph.add_nodes_from(range(G))
    graph.add_edges_from((j, i) for j in range(G) for i in range(G) if adj[j, i])
    group = SVGPathGroup([square_path(bool(c)) for c in cw], fill=True)
    group.overlap_graph = lambda *a, **k: graph
    group.compute_filling()
    return [int(p.filling) for p in group.svg_paths]


def forest(rng):
    """transitive closure of a random forest under a random labelling: adj[a, d] = 1 for every ancestor a of d"""
    label = rng.permutation(G)
    parent = [-1 if (k == 0 or rng.random() < 0.3) else int(rng.integers(0, k)) for k in range(G)]
    adj = np.zeros((G, G), dtype=np.uint8)
    for k in range(G):
        a = parent[k]
        while a >= 0:
            adj[label[a], label[k]] = 1
            a = parent[a]
    return adj


def random_digraph(rng, p=0.15):
    adj = (rng.random((G, G)) < p).astype(np.uint8)
    adj[np.arange(G), np.arange(G)] = 0
    return adj


def restated(adj, cw, order):
    area, inter = FR.counts_from_adjacency(adj)
    r = FR.filling_from_counts(area, inter, cw, [True] * G, 0.9, "orientation", order=order)
    return r["filling"], r


if __name__ == "__main__":
    rng = np.random.default_rng(2025)
    cases = [(forest(rng), 0) for _ in range(150)] + [(random_digraph(rng), 1) for _ in range(350)]
    adjs, cws, fams, frees, fills = [], [], [], [], []
    for adj, fam in cases:
        cw = rng.random(G) < 0.5
        up, full_up = restated(adj, cw, "ascending")
        down, full_down = restated(adj, cw, "descending")
        free = full_up == full_down
        ref = reference(adj, cw)
        if free:
            assert ref == up, (adj, cw, ref, up)
        if fam == 0:
            assert free, "a forest whose result depends on the order inside a level"
        adjs.append((adj << np.arange(G, dtype=np.uint8)[None, :]).sum(1).astype(np.uint8))
        cws.append(cw), fams.append(fam), frees.append(free), fills.append(ref)
    fams, frees = np.array(fams, dtype=np.uint8), np.array(frees)
    share = frees[fams == 1].mean()
    assert share >= 0.95, share
    fills = np.array(fills, dtype=np.int8)
    assert (fills == 2).any() and (fills == 0).any() and (fills == 1).any()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "filling.npz")
    np.savez_compressed(path, adj=np.stack(adjs), clockwise=np.stack(cws), family=fams, order_free=frees, filling=fills)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases; order-free share of the random family",
          f"{share:.4f}; erase paths in {int((fills == 2).any(1).sum())} cases, unreached groups in "
          f"{int((fills == 0).any(1).sum())}")
