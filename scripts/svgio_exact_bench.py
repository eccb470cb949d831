"""Micro-timing of the two number rules of svgio.parse_paths (dsvg_svg_parse / dsvg_svg_parse_exact) in one process, with the
conventions of scripts/svgio_bench.py: device events, warm-up, the median over 7 rounds of the mean of 50 eager calls, 512 and
8,192 strings made by repeating strings of tests/golden/svgio/parse.npz, one string per icon (G = 1, S = 512).  Within a round
the sides of a comparison run one after the other, so that a drift of the box hits both:
  (a) the fast entry on the strings that give rows there (flag 0): this build against another build of the library, given with
      --parent-lib (the parent commit's libdsvg_hip.so, built there with deepsvg_amd/csrc/build.sh).  Both are called through
      the C entry itself on the same buffers.  Condition: the difference of the medians lies inside the spread of the parent's
      own rounds.  Without --parent-lib this part is left out.
  (b) the exact entry against the fast entry on the same all-fast strings: the ratio of the medians.
  (c) the exact entry on the 30 strings with long numbers (flag 3 without "slow: 25 digits"), repeated, against
      - the fast entry on the same strings with every number cut to 15 significant digits (same tokens, same rows), which
        isolates the cost of the conversion;
      - the restatement with float() as its decimal rule on one core.
Nothing of the reference is read.  Prints the figures and writes them to --log (default profiles/svgio_exact_bench.log)."""
import argparse
import ctypes
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import lib, svgio                  # noqa: E402
from tests import svgio_ref as R                    # noqa: E402

NUMBER = re.compile(rb"[-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?")
S = 512


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # microseconds


def alternate(sides, reps, rounds):
    """{name: fn} -> {name: [microseconds per round]}, the sides one after the other within every round"""
    for fn in sides.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            out[k].append(timed(fn, reps))
    return out


def show(times):
    return f"{statistics.median(times):.1f} us [{min(times):.1f} .. {max(times):.1f}]"


def raw_entry(handle, symbol, dev, P):
    """the C entry `symbol` of the library `handle` on preallocated outputs -> a function of no arguments"""
    fn = getattr(handle, symbol)
    fn.restype, fn.argtypes = lib.SIGNATURES[symbol]
    data, off, kind, slot = dev
    out = [torch.empty(P, 1, S, device="cuda"), torch.empty(P, 1, S, 11, device="cuda"), torch.empty(P, 1, dtype=torch.int32, device="cuda"),
           torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(P, dtype=torch.bool, device="cuda")]
    ws = torch.empty(2 * P, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (data.data_ptr(), data.numel(), off.data_ptr(), kind.data_ptr(), slot.data_ptr(), P, P, 1, S, ws.data_ptr(),
            *(t.data_ptr() for t in out), stream)

    def call():
        if fn(*args) != 0:
            raise RuntimeError(symbol)
    call.out, call.keep = out, (ws, dev)             # the pointers in `args` stay valid as long as the function lives
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "svgio_exact_bench.log"))
    ap.add_argument("--parent-lib", default=None, help="libdsvg_hip.so of the commit to compare the fast entry with")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svgio_exact_bench: needs a GPU (a CPU run measures nothing)")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "svgio", "parse.npz"))
    data = gold["data"].tobytes()
    text = lambda p: data[gold["offsets"][p]:gold["offsets"][p + 1]]       # noqa: E731
    fast_ids = [p for p in range(len(gold["kind"])) if gold["flag"][p] == 0]
    long_ids = [p for p in range(len(gold["kind"])) if gold["flag"][p] == 3 and gold["tag"][p] != "slow: 25 digits"]
    fast_strings, fast_kinds = [text(p) for p in fast_ids], gold["kind"][fast_ids]
    long_strings = [text(p) for p in long_ids]
    def cut(m):                                      # 15 digits; 1.5 for the two numbers whose exponent alone is outside the fast rule
        short = b"%.15g" % float(m.group(0))
        return short if R.decimal(short) is not None else b"1.5"

    cut_strings = [NUMBER.sub(cut, s) for s in long_strings]
    numbers = sum(len(NUMBER.findall(s)) for s in long_strings)
    assert len(long_strings) == 30 and all(len(NUMBER.findall(c)) == len(NUMBER.findall(s)) for c, s in zip(cut_strings, long_strings))
    lines = [f"{torch.cuda.get_device_name(0)}; G=1, S={S}; microseconds per call: median of {a.rounds} rounds, each the mean of "
             f"{a.reps} eager calls, [min .. max] over the rounds; the sides of a comparison alternate within every round",
             f"all-fast strings: the {len(fast_strings)} strings of tests/golden/svgio/parse.npz with flag 0 ({sum(map(len, fast_strings))} "
             f"bytes), repeated; long strings: its {len(long_strings)} strings with flag 3 that the exact rule reads "
             f"({sum(map(len, long_strings))} bytes, {numbers} numbers), repeated"]
    mine = lib.load()
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    # the restatement with float() on one core, once on the distinct long strings
    torch.set_num_threads(1)
    own, R.decimal = R.decimal, lambda t: float(t)
    t0 = time.perf_counter()
    for s in long_strings:
        assert R.parse(s, 0, S)[0] == R.OK
    ref_float_s = time.perf_counter() - t0
    R.decimal = own
    for P in (512, 8192):
        def packed(strings, kinds):
            idx = np.arange(P) % len(strings)
            host_data, host_off = svgio.pack_strings([strings[i] for i in idx])
            return [torch.from_numpy(x).cuda() for x in (host_data, host_off, np.asarray(kinds)[idx].astype(np.uint8),
                                                         np.arange(P, dtype=np.int32))]
        dev_fast = packed(fast_strings, fast_kinds)
        dev_long, dev_cut = packed(long_strings, np.zeros(30, np.uint8)), packed(cut_strings, np.zeros(30, np.uint8))
        # (a)
        if parent is not None:
            new_fn, old_fn = raw_entry(mine, "dsvg_svg_parse", dev_fast, P), raw_entry(parent, "dsvg_svg_parse", dev_fast, P)
            t = alternate({"parent": old_fn, "this": new_fn}, a.reps, a.rounds)
            names = ("commands", "args", "len_groups", "status", "valid")
            bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x          # noqa: E731
            differ = [n for n, x, y in zip(names, new_fn.out, old_fn.out) if not torch.equal(bits(x), bits(y))]
            assert int(new_fn.out[3].sum()) == 0, "this build: a status that is not OK"
            diff = statistics.median(t["this"]) - statistics.median(t["parent"])
            spread = max(t["parent"]) - min(t["parent"])
            lines.append(f"(a) {P} all-fast strings, dsvg_svg_parse through the C entry: parent build {show(t['parent'])}, this build "
                         f"{show(t['this'])}; difference of the medians {diff:+.1f} us, spread of the parent's rounds {spread:.1f} us: "
                         f"{'inside' if abs(diff) <= spread else 'OUTSIDE'} the spread; " + ("identical bits" if not differ else "outputs that DIFFER: " + ", ".join(differ)))
        # (b)
        quick = lambda: svgio.parse_paths(*dev_fast, N=P, G=1, S=S)                          # noqa: E731
        exact = lambda: svgio.parse_paths(*dev_fast, N=P, G=1, S=S, numbers="exact")         # noqa: E731
        t = alternate({"fast": quick, "exact": exact}, a.reps, a.rounds)
        rq, rx = quick(), exact()
        assert int(rx["status"].sum()) == 0 and torch.equal(rq["args"].view(torch.int32), rx["args"].view(torch.int32))
        ratio = statistics.median(t["exact"]) / statistics.median(t["fast"])
        spread = max(t["fast"]) - min(t["fast"])
        lines.append(f"(b) {P} all-fast strings, parse_paths: fast entry {show(t['fast'])}, exact entry {show(t['exact'])}; exact / fast = "
                     f"{ratio:.3f}, difference {statistics.median(t['exact']) - statistics.median(t['fast']):+.1f} us, spread of the fast "
                     f"entry's rounds {spread:.1f} us")
        # (c)
        exact_long = lambda: svgio.parse_paths(*dev_long, N=P, G=1, S=S, numbers="exact")    # noqa: E731
        quick_cut = lambda: svgio.parse_paths(*dev_cut, N=P, G=1, S=S)                       # noqa: E731
        t = alternate({"cut": quick_cut, "exact": exact_long}, a.reps, a.rounds)
        rl, rc = exact_long(), quick_cut()
        assert int(rl["status"].sum()) == 0 and int(rc["status"].sum()) == 0 and torch.equal(rl["len_groups"], rc["len_groups"])
        assert int((svgio.parse_paths(*dev_long, N=P, G=1, S=S)["status"] == R.SLOW_NUMBER).sum()) == P
        med = statistics.median(t["exact"])
        per = (med - statistics.median(t["cut"])) * 1e3 / (numbers * P / 30)
        lines.append(f"(c) {P} long strings ({numbers * P // 30} numbers), parse_paths: exact entry {show(t['exact'])}; fast entry on the "
                     f"same strings with every number cut to 15 digits {show(t['cut'])}; exact / cut = "
                     f"{med / statistics.median(t['cut']):.3f} ({per:.2f} ns per number more); the restatement with float() on one core "
                     f"{ref_float_s * P / 30 * 1e3:.0f} ms = {ref_float_s * P / 30 * 1e6 / med:.0f}x the exact entry (measured once on the 30 "
                     f"strings: {ref_float_s * 1e3:.1f} ms, scaled by the repeats)")
    out = "\n".join(lines)
    print(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write(out + "\n")


if __name__ == "__main__":
    main()
