"""Micro-timing of SVG text -> tensors (svgio.parse_paths: dsvg_svg_parse, five launches) in one process, on 512 and 8,192 strings
made by repeating the strings of tests/golden/svgio/parse.npz that give rows, one string per icon (G = 1, S = 512):
  (a) parse_paths on packed tensors that are on the device already: the median over the rounds of the mean of `reps` eager calls
      between two device events, the spread the range over the rounds; with it the algorithmic bytes per second, where the
      bytes are the text in plus the rows out (48 per row), and the bytes the call really writes (the padded groups);
  (b) the restatement tests/svgio_ref.py on the distinct strings on one core, as it is and with float() in place of its decimal
      rule, scaled by the number of repeats;
  (c) load_svgs whole on documents of four of these paths each (wall clock around a synchronize), and the host's XML pass over
      the same documents alone.
Nothing of the reference is read.  Prints the figures and writes them to --log (default profiles/svgio_bench.log)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepsvg_amd import svgio                       # noqa: E402
from tests import svgio_ref as R                    # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "svgio_bench.log"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svgio_bench: needs a GPU (a CPU run measures nothing)")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "svgio", "parse.npz"))
    data = gold["data"].tobytes()
    keep = [p for p in range(len(gold["kind"])) if gold["flag"][p] == 0]
    strings = [data[gold["offsets"][p]:gold["offsets"][p + 1]] for p in keep]
    kinds = gold["kind"][keep]
    rows = np.diff(gold["row_offsets"])[keep]
    S = 512
    lines = [f"{torch.cuda.get_device_name(0)}; {len(strings)} distinct strings of tests/golden/svgio/parse.npz "
             f"({sum(map(len, strings))} bytes, {int(rows.sum())} rows), repeated; G=1, S={S}; microseconds per call: median of "
             f"{a.rounds} rounds, each the mean of {a.reps} eager calls; [min .. max] over the rounds"]
    # (b) the restatement on one core
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for s, k in zip(strings, kinds):
        R.parse(s, int(k), S)
    ref_s = time.perf_counter() - t0
    own, R.decimal = R.decimal, lambda text: float(text)
    t0 = time.perf_counter()
    for s, k in zip(strings, kinds):
        R.parse(s, int(k), S)
    ref_float_s = time.perf_counter() - t0
    R.decimal = own
    for P in (512, 8192):
        idx = np.arange(P) % len(strings)
        host_data, host_off = svgio.pack_strings([strings[i] for i in idx])
        dev = [torch.from_numpy(x).cuda() for x in (host_data, host_off, kinds[idx].astype(np.uint8), np.arange(P, dtype=np.int32))]
        fn = lambda: svgio.parse_paths(*dev, N=P, G=1, S=S)      # noqa: E731
        for _ in range(5):
            res = fn()
        torch.cuda.synchronize()
        assert int((res["status"] != 0).sum()) == 0 and int(res["len_groups"].sum()) == int(rows[idx].sum())
        times = [timed(fn, a.reps) for _ in range(a.rounds)]
        med = statistics.median(times)
        alg = len(host_data) + int(rows[idx].sum()) * 48
        wrote = P * S * 48 + P * 12
        lines.append(f"{P} strings ({len(host_data)} bytes of text, {int(rows[idx].sum())} rows) parse_paths: {med:.1f} us "
                     f"[{min(times):.1f} .. {max(times):.1f}]; text in + rows out {alg} bytes = {alg / med / 1e3:.2f} GB/s; written with "
                     f"the padding {wrote} bytes = {wrote / med / 1e3:.1f} GB/s")
        lines.append(f"{P} strings, tests/svgio_ref.py on one core: {ref_s * P / len(strings) * 1e3:.0f} ms "
                     f"({ref_s * P / len(strings) * 1e6 / med:.0f}x the kernel); with float() for its decimal rule "
                     f"{ref_float_s * P / len(strings) * 1e3:.0f} ms (measured once on the distinct strings: {ref_s * 1e3:.0f} ms and "
                     f"{ref_float_s * 1e3:.0f} ms, scaled by the repeats)")
        # (c) documents of four paths each
        paths_only = [i for i in idx if kinds[i] == 0][: P // 4 * 4]
        docs = []
        for n in range(len(paths_only) // 4):
            body = "".join(f'<path d="{strings[i].decode("utf-8")}"/>' for i in paths_only[4 * n:4 * n + 4])
            docs.append(f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 24 24">{body}</svg>')
        for _ in range(2):
            svgio.load_svgs(docs, max_num_groups=4, max_seq_len=S - 2)
        torch.cuda.synchronize()
        whole, xml = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            svgio.load_svgs(docs, max_num_groups=4, max_seq_len=S - 2)
            torch.cuda.synchronize()
            whole.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for d in docs:
                svgio._document(d)
            xml.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"{len(docs)} documents of 4 paths ({sum(map(len, docs))} bytes) load_svgs: {statistics.median(whole):.1f} ms "
                     f"[{min(whole):.1f} .. {max(whole):.1f}], of which the host's XML pass {statistics.median(xml):.1f} ms "
                     f"({100 * statistics.median(xml) / statistics.median(whole):.0f} %)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
