"""The exact number rule of deepsvg_amd.svgio without a GPU: its restatement (tests/svgio_exact_ref.py) against float() by bits,
against the fast rule where that applies and against the reference's own rows (tests/golden/svgio/exact.npz); the header
deepsvg_amd/csrc/decimal_exact.h on its own in a host program against strtod; and the Python surface (`numbers="fast" | "exact"`)
against a fake `ops` that runs the restatement."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from deepsvg_amd import lib, svgio
from deepsvg_amd.svgtensor import CMD_ARGS_MASK
from deepsvg_amd.synthetic import make_batch
from tests import svgio_exact_ref as X
from tests import svgio_ref as R

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "svgio", "parse.npz")
GOLD_EXACT = os.path.join(HERE, "golden", "svgio", "exact.npz")
ROWS, RAISES, EMPTY, SLOW = range(4)                 # the flags of both golden files
# the directed numbers of tests/golden/make_golden_svgio_exact.py
DIRECTED = ["0.12345678901234567", "123456789012345678", "1234567890123456789", "9999999999999999999", "12345678901234567890",
            "9007199254740991", "9007199254740992", "9007199254740993", "18014398509481985", "18014398509481987", "1e-64",
            "9999999999999999999e-64", "1e38", "9999999999999999999e38", "0.01e-62", "300e36", "0." + "0" * 30 + "123",
            "0." + "0" * 30 + "1234567890123456789", "." + "0" * 30 + "5e31", "7" + "0" * 25, "1234567890123456789" + "0" * 25,
            "5" + "0" * 25 + ".000e-24", "1e23", "1.5e-30", "-5.9604644775390625e-08", "1.0000000000000000", "0.99999999999999999",
            "1.9999999999999998", "30.000000000000004", "10000000000000000e-16", "3.4028234663852886e+38", "1e-45", "4.35", "0.1"]


def strings_of(gold):
    data = gold["data"].tobytes()
    return [data[gold["offsets"][p]:gold["offsets"][p + 1]] for p in range(len(gold["kind"]))]


def spelled(rng, digits, e10):
    """the digits of w (first and last not 0) with 10^e10, spelled one of several ways"""
    nd = len(digits)
    style = rng.randint(0, 4)
    if style == 0 and -40 <= e10 <= 0:               # a plain fraction
        body = digits[:nd + e10] + "." + digits[nd + e10:] if -e10 < nd else ["0.", "."][rng.randint(0, 2)] + "0" * (-e10 - nd) + digits
        body += "0" if body.endswith(".") else ""
    elif style == 1 and 0 <= e10 <= 30:              # a plain integer, with zeros behind the dot or without
        body = digits + "0" * e10 + ["", ".0", ".000"][rng.randint(0, 3)]
    else:                                            # exponent form, the dot anywhere
        cut = rng.randint(0, nd + 1)
        body = digits[:cut] + ("." + digits[cut:] if cut < nd or rng.randint(0, 2) else "")
        body += "0" if body.endswith(".") else ""
        if rng.randint(0, 3) == 0:                   # trailing zeros of the fraction
            body += ("" if "." in body else ".") + "0" * rng.randint(1, 5)
        body += ["e%+d", "E%d"][rng.randint(0, 2)] % (e10 + nd - cut)
    if rng.randint(0, 3) == 0:
        body = "0" * rng.randint(1, 5) + body        # leading zeros
    return ["", "-", "+"][rng.randint(0, 3)] + body


def same_bits(text):
    got = X.decimal_exact(text.encode())
    assert got is not None and R.f64_bits(got) == R.f64_bits(float(text)), (text, got)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_decimal_exact_equals_float_on_200k_seeded_texts_and_the_fast_rule_where_it_applies():
    rng = np.random.RandomState(19)
    n, fast = 200000, 0
    nds = rng.randint(1, X.DIGITS + 1, n)
    e10s = np.where(rng.randint(0, 3, n) > 0, rng.randint(X.E10_MIN, X.E10_MAX + 1, n), -rng.randint(0, 24, n))
    for i in range(n):
        digits = "".join(map(str, rng.randint(0, 10, nds[i])))
        digits = str(rng.randint(1, 10)) + digits[1:-1] + (str(rng.randint(1, 10)) if nds[i] > 1 else "")
        text = spelled(rng, digits, int(e10s[i]))
        same_bits(text)
        quick = R.decimal(text.encode())
        if quick is not None:
            fast += 1
            assert R.f64_bits(quick) == R.f64_bits(X.decimal_exact(text.encode())), text
    assert n // 10 < fast < n - n // 10               # both sides of the fast rule's border are well covered
    for text in DIRECTED:
        same_bits(text)
        same_bits("-" + text.lstrip("-"))
    for _ in range(2000):                             # exact midpoints between neighbouring doubles, and their neighbours
        m = (1 << 52) | int(rng.randint(0, 2 ** 31)) << 21 | int(rng.randint(0, 2 ** 21))
        mid = (2 * m + 1) << int(rng.randint(0, 10))
        for v in (mid - 1, mid, mid + 1):
            same_bits(str(v))
            same_bits("%de%d" % (v, rng.randint(-40, 20)))
    for v in rng.uniform(-1, 1, 20000).astype(F) * F(10.0) ** rng.randint(-12, 7, 20000).astype(F):
        same_bits(repr(float(v)))                     # as save_svg prints a float32


def test_decimal_exact_outside_the_domain_and_zeros():
    for text in (b"12345678901234567891", b"1.2345678901234567891", b"0.00012345678901234567891", b"1e-65", b"1e39", b"10e38",
                 b"0.1e-64", b"9999999999999999999e39", b"1234567890123456789012345", b"1e999", b"1e-999", b"1e99999999999"):
        assert X.decimal_exact(text) is None, text
    assert X.split(b"-00120.0340e5") == (True, 120034, 6, 2) and X.split(b"1200") == (False, 12, 2, 2)
    assert X.split(b"12345678901234567890")[1:] == (1234567890123456789, 19, 1)             # a trailing zero is no digit of w
    assert X.decimal_exact(b"12345678901234567890") == 12345678901234567890.0
    for text, neg in ((b"0", 0), (b"-0", 1), (b"0e999", 0), (b"-0.000e-999", 1), (b"+.0", 0), (b"-000.000E5", 1)):
        assert R.f64_bits(X.decimal_exact(text)) == neg << 63, text
    assert (X.DIGITS, X.E10_MIN, X.E10_MAX) == (19, -64, 38) and 10 ** X.DIGITS < 2 ** 64
    assert (5 ** X.E10_MAX).bit_length() == 89 and (5 ** -X.E10_MIN).bit_length() == 149
    # below the domain a number is zero in float32, above it infinite
    with np.errstate(over="ignore"):
        assert F(float("9999999999999999999e-65")) == 0 and np.isinf(F(float("1e39")))


# ---- the restatement, against the reference's rows ---------------------------------------------------------------------------------------
def test_restatement_in_exact_mode_equals_the_reference_on_exact_npz():
    gold = dict(np.load(GOLD_EXACT))
    flags, tags = gold["flag"], gold["tag"]
    assert len(flags) >= 150 and (flags == ROWS).sum() >= 140 and (flags == SLOW).sum() >= 8
    assert {"integer", "midpoint", "e10 inside", "e10 outside", "30 leading zeros", "25 trailing zeros", "zero", "arc flags",
            "relative chain", "docs slow", "slow: 25 digits"} <= set(tags.tolist())
    slow_there = 0
    for p, s in enumerate(strings_of(gold)):
        kind = int(gold["kind"][p])
        st, cmd, args = X.parse(s, kind, numbers="exact")
        lo, hi = gold["row_offsets"][p], gold["row_offsets"][p + 1]
        what = (p, tags[p], s[:60])
        if flags[p] == ROWS:
            assert st == R.OK and np.array_equal(cmd, gold["commands"][lo:hi]), what
            assert np.array_equal(R.bits(args), R.bits(gold["args"][lo:hi])), what
        else:
            assert flags[p] == SLOW and st == R.SLOW_NUMBER and len(cmd) == 0, what
        quick = X.parse(s, kind, numbers="fast")
        own = R.parse(s, kind)
        assert quick[0] == own[0] and np.array_equal(quick[1], own[1]) and np.array_equal(R.bits(quick[2]), R.bits(own[2])), what
        slow_there += own[0] == R.SLOW_NUMBER
        if own[0] == R.OK:                               # where the fast rule reads a string the exact rule reads the same rows
            assert st == R.OK and np.array_equal(R.bits(args), R.bits(own[2])), what
    assert slow_there >= 140
    with pytest.raises(ValueError):
        X.parse(b"M1 2", numbers="slow")


def test_restatement_in_exact_mode_on_parse_npz():
    gold = dict(np.load(GOLD))
    strings, flags, tags = strings_of(gold), gold["flag"], gold["tag"]
    ok = 0
    for p in np.flatnonzero(flags == SLOW):
        st = X.parse(strings[p], int(gold["kind"][p]), numbers="exact")[0]
        assert st == (R.SLOW_NUMBER if tags[p] == "slow: 25 digits" else R.OK), tags[p]
        ok += st == R.OK
    assert ok == 30 and (flags == SLOW).sum() == 31
    for p in np.flatnonzero(flags != SLOW):
        a, b = X.parse(strings[p], int(gold["kind"][p]), numbers="exact"), R.parse(strings[p], int(gold["kind"][p]))
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(R.bits(a[2]), R.bits(b[2])), tags[p]


# ---- the header on its own ------------------------------------------------------------------------------------------------------------
def test_the_header_on_its_own_against_strtod_under_sanitizers(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = os.path.join(HERE, "decimal_exact_check.cpp"), str(tmp_path / "decimal_exact_check")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    san = ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:
        print("the sanitizer runtimes do not link here; building plain:\n" + built.stderr[-400:])
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    ran = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=600)
    print(ran.stdout[-600:])
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    m = re.search(r"(\d+) texts, 0 failures", ran.stdout)
    assert m and int(m.group(1)) >= 1000000


# ---- the Python surface, against a fake ops that runs the restatement -------------------------------------------------------------------
class _FakeOps:
    def __init__(self):
        self.fast, self.exact = [], []

    def require_device(self, device):
        pass

    def svg_parse(self, data, offsets, kind, slot, N, G, S):                # seven positional arguments and no more
        self.fast.append((data, offsets, kind, slot, N, G, S))
        return {k: torch.from_numpy(v) for k, v in R.parse_paths(data.numpy(), offsets.numpy(), kind.numpy(), slot.numpy(), N, G, S).items()}

    def svg_parse_exact(self, data, offsets, kind, slot, N, G, S):
        self.exact.append((data, offsets, kind, slot, N, G, S))
        res = X.parse_paths(data.numpy(), offsets.numpy(), kind.numpy(), slot.numpy(), N, G, S, numbers="exact")
        return {k: torch.from_numpy(v) for k, v in res.items()}


@pytest.fixture
def fake_ops(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(svgio, "ops", fake)
    return fake


def generic_batch(n, seed=5):
    """`make_batch` with every enabled argument times float32 0.1: make_batch draws integers, which print short; these are
    float32 values as a decoded or preprocessed icon holds them, and repr() prints them with 16 or 17 digits"""
    cmd, args = make_batch(n, seed=seed)
    on = CMD_ARGS_MASK[cmd.long()].bool()
    return cmd, torch.where(on, args * torch.tensor(0.1, dtype=torch.float32), args)


def saved_documents(cmd, args):
    """tensors -> documents with every number printed as the reference's save_svg prints a float32: repr(float(x))"""
    cmd, args = cmd.numpy(), args.numpy()
    mask = CMD_ARGS_MASK.numpy().astype(bool)
    docs = []
    for n in range(cmd.shape[0]):
        body = ""
        for g in range(cmd.shape[1]):
            parts = []
            for r in range(1, cmd.shape[2]):
                c = int(cmd[n, g, r])
                if c == R.EOS:
                    break
                parts.append("MLCA..Z"[c] + " ".join(repr(float(v)) for v in args[n, g, r][mask[c]]))
            body += '<path fill="none" d="%s"/>' % " ".join(parts)
        docs.append('<svg xmlns="http://www.w3.org/2000/svg" viewBox="0.0 0.0 24.0 24.0">%s</svg>' % body)
    return docs


def test_saved_float32_text_reads_back_bit_for_bit_with_exact_numbers(fake_ops):
    cmd, args = generic_batch(8)
    docs = saved_documents(cmd, args)
    assert max(len(t) for t in re.findall(r"[0-9.]+", docs[0])) >= 18             # 17 digits and a dot
    res = svgio.load_svgs(docs, max_num_groups=8, max_seq_len=30, device="cpu", numbers="exact")
    assert res["valid"].all() and torch.equal(res["commands"], cmd)
    assert np.array_equal(R.bits(res["args"].numpy()), R.bits(args.numpy()))
    assert (res["status"] <= R.EMPTY).all() and len(fake_ops.exact) == 1 and not fake_ops.fast
    quick = svgio.load_svgs(docs, max_num_groups=8, max_seq_len=30, device="cpu")
    assert not quick["valid"].any() and (quick["status"] == R.SLOW_NUMBER).sum() >= 8
    assert set(quick["status"].tolist()) <= {R.SLOW_NUMBER, R.OK, R.EMPTY} and len(fake_ops.fast) == 1


def test_numbers_chooses_the_entry_and_is_forwarded(fake_ops, monkeypatch, tmp_path):
    svgio.parse_paths(["M1 2L3 4"], G=1, S=4, device="cpu")
    assert len(fake_ops.fast) == 1 and len(fake_ops.fast[0]) == 7 and not fake_ops.exact
    svgio.parse_paths(["M1 2L3 4"], G=1, S=4, device="cpu", numbers="fast")
    assert len(fake_ops.fast) == 2 and not fake_ops.exact
    slow = "M0.12345678901234567 1L2 3"
    res = svgio.parse_paths([slow], G=1, S=4, device="cpu", numbers="exact")
    assert len(fake_ops.exact) == 1 and len(fake_ops.fast) == 2 and res["status"].tolist() == [R.OK]
    assert svgio.parse_paths([slow], G=1, S=4, device="cpu")["status"].tolist() == [R.SLOW_NUMBER]
    t = lambda a, dt: torch.tensor(a, dtype=dt)                       # noqa: E731
    tensors = (t(list(slow.encode()), torch.uint8), t([0, len(slow)], torch.int64), t([0], torch.uint8), t([0], torch.int32))
    assert svgio.parse_paths(*tensors, N=1, G=1, S=4, numbers="exact")["status"].tolist() == [R.OK] and len(fake_ops.exact) == 2
    doc = f'<svg viewBox="0 0 24 24"><path d="{slow}"/><rect width="1.0000000000000000001" height="2"/></svg>'
    assert svgio.load_svgs([doc], 2, 6, "cpu")["valid"].tolist() == [False]
    both = svgio.load_svgs([doc], 2, 6, "cpu", numbers="exact")
    assert both["valid"].tolist() == [True] and both["len_groups"].tolist() == [[2, 6]] and len(fake_ops.exact) == 3
    # preprocess_files hands the choice to load_svgs
    seen = []

    def load(texts, max_num_groups, max_seq_len, device, numbers="fast"):
        seen.append(numbers)
        raise RuntimeError("far enough")

    monkeypatch.setattr(svgio, "load_svgs", load)
    f = tmp_path / "a.svg"
    f.write_text(doc)
    for kw, want in (({}, "fast"), ({"numbers": "exact"}, "exact")):
        with pytest.raises(RuntimeError, match="far enough"):
            svgio.preprocess_files([str(f)], device="cpu", **kw)
        assert seen[-1] == want
    monkeypatch.undo()
    monkeypatch.setattr(svgio, "ops", fake_ops)
    calls = len(fake_ops.fast) + len(fake_ops.exact)
    for bad in ("slow", "EXACT", None, 1, True):
        with pytest.raises(ValueError):
            svgio.parse_paths(["M1 2L3 4"], G=1, S=4, device="cpu", numbers=bad)
        with pytest.raises(ValueError):
            svgio.load_svgs([doc], 2, 6, "cpu", numbers=bad)
        with pytest.raises(ValueError):
            svgio.preprocess_files([str(f)], device="cpu", numbers=bad)
    assert len(fake_ops.fast) + len(fake_ops.exact) == calls


def test_binding_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "dsvg.h")).read()
    decl = re.search(r"int dsvg_svg_parse_exact\(([^)]*)\);", hdr).group(1)
    fast = re.search(r"int dsvg_svg_parse\(([^)]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 16 and [a.split() for a in decl.split(",")] == [a.split() for a in fast.split(",")]
    assert lib.SIGNATURES["dsvg_svg_parse_exact"] == lib.SIGNATURES["dsvg_svg_parse"] and len(lib.SIGNATURES["dsvg_svg_parse_exact"][1]) == 16
    assert lib.ABI_VERSION == int(re.search(r"#define DSVG_ABI_VERSION (\d+)", hdr).group(1)) == 19
    for name, ref in (("DIGITS", X.DIGITS), ("E10_MIN", X.E10_MIN), ("E10_MAX", X.E10_MAX)):
        value = int(re.search(r"#define DSVG_SVG_EXACT_%s \(?(-?\d+)\)?" % name, hdr).group(1))
        assert getattr(lib, "DSVG_SVG_EXACT_" + name) == value == ref, name
    src = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "svg_parse.hip")).read()
    assert "svg_parse_kernel<EXACT>" in src and '#include "decimal_exact.h"' in src
    own = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "decimal_exact.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)', own) == ["stdint.h", "../../include/dsvg.h"]           # nothing of HIP
