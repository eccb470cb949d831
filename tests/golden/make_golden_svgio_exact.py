"""Generates tests/golden/svgio/exact.npz by running the REAL reference parser, `deepsvg.svglib.svg_path.SVGPath.from_str(s)
.to_tensor()` (and the polygon / polyline `points` reader), on path strings whose numbers are long: outside the fast rule of
include/dsvg.h and, most of them, inside its exact rule.  Run in the build container only, like make_golden_svgio.py, whose
stubs and whose `reference()` it uses:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_svgio_exact.py

Stored, in the layout of parse.npz: the strings as bytes with offsets, kinds and a tag each; a flag per string (0 rows, 1 the
reference raises, 2 an empty group, 3 a number the reference converts is outside the EXACT domain: more than 19 significant
digits, or a decimal exponent below -64 or above 38); the reference's rows under CMD_ARGS_MASK.  The strings:
 - the 31 strings of parse.npz with flag 3 there (five named ones and the `d` strings of the reference's docs/ that hold 17-digit
   numbers); all but "slow: 25 digits" have rows here;
 - grammar strings: float32 values printed through float64 with repr(), the way the reference's save_svg prints them, across the
   magnitudes 1e-12 .. 1e6; 18-, 19- and 20-digit integers and 2^53 +- 1; exact midpoints between neighbouring doubles and their
   neighbours; the decimal exponents -65, -64, 38 and 39; fractions with 30 leading zeros; integers with 25 trailing zeros;
   0e999 and -0.000e-999; long numbers as arc flags and in h / v / relative chains.
No reference code and no reference file is stored: only path strings and result tensors."""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_svgio as G                        # noqa: E402  (stubs the drawing stack, imports the reference)
from tests import svgio_exact_ref as X               # noqa: E402
from tests import svgio_ref as R                     # noqa: E402

ROWS, RAISES, EMPTY, SLOW = range(4)
F = np.float32


def long_form(v):
    """a float32 value as save_svg prints it: through float64, with repr()"""
    return repr(float(F(v)))


def inside(s, kind):
    """every number the reference converts is inside the exact domain"""
    data = s.encode("utf-8")
    seen = kind != R.KIND_PATH
    for tok in R.tokens(data, kind):
        if tok[0] == "c":
            seen = True
        elif seen and X.decimal_exact(data[tok[1]:tok[2]]) is None:
            return False
    return True


def slow_of_parse_npz():
    gold = np.load(os.path.join(HERE, "svgio", "parse.npz"))
    data = gold["data"].tobytes()
    return [(str(gold["tag"][p]), data[gold["offsets"][p]:gold["offsets"][p + 1]].decode("utf-8"), int(gold["kind"][p]))
            for p in range(len(gold["kind"])) if gold["flag"][p] == SLOW]


def grammar_strings():
    rng = np.random.RandomState(20240917)
    P = R.KIND_PATH
    out = []

    def values(mag, k):
        return [long_form(rng.uniform(-1, 1) * 10.0 ** mag) for _ in range(k)]

    for mag in range(-12, 7):                                   # save_svg's numbers, magnitude by magnitude
        a = values(mag, 16)
        out.append((f"repr 1e{mag}", "M{} {}L{} {}C{} {} {} {} {} {}z".format(*a[:10]), P))
        out.append((f"repr 1e{mag} relative", "m{} {}l{} {} {} {}c{} {} {} {} {} {}".format(*a[:12]), P))
        out.append((f"repr 1e{mag} glued", "M" + "".join((v if v[0] == "-" else " " + v) for v in a[:2]) + "h" + a[2] + "v" + a[3]
                    + "s" + ",".join(a[4:8]) + "q" + " ".join(a[8:12]) + "t" + " ".join(a[12:14]), P))
    for mag in (-6, 0, 3):
        out.append((f"repr 1e{mag} points", " ".join(values(mag, 12)), R.KIND_POLYGON))
        out.append((f"repr 1e{mag} points", ",".join(values(mag, 8)), R.KIND_POLYLINE))
    for _ in range(6):                                          # mixed magnitudes, the exponent form repr() chooses below 1e-4
        a = [long_form(rng.uniform(-1, 1) * 10.0 ** rng.randint(-12, 7)) for _ in range(14)]
        out.append(("repr mixed", "M{} {}l{} {}h{}v{}c{} {} {} {} {} {}L{} {}".format(*a), P))
    integers = ["123456789012345678", "999999999999999999", "1234567890123456789", "9999999999999999999", "12345678901234567890",
                "12345678901234567891", "9007199254740991", "9007199254740992", "9007199254740993", "18014398509481985"]
    for n in integers:
        out.append(("integer", f"M{n}e-14 1L2 -{n}e-17", P))
        out.append(("integer", f"M1 2l{n}E-18 +{n}e-19", P))
    for _ in range(12):                                         # exact midpoints between doubles, and their neighbours
        m = (1 << 52) | int(rng.randint(0, 2 ** 31)) << 21 | int(rng.randint(0, 2 ** 21))
        mid = (2 * m + 1) << int(rng.randint(0, 10))
        out.append(("midpoint", f"M{mid - 1}e-16 {mid}e-16L{mid + 1}e-16 -{mid}e-18", P))
    for lo, hi in (("1e-65", "1e-64"), ("9999999999999999999e-65", "9999999999999999999e-64"), ("1e39", "1e38"),
                   ("20e38", "2e38"), ("0.001e-62", "0.01e-62"), ("3000e36", "300e36")):
        out.append(("e10 outside", f"M1 2L{lo} 3", P))
        out.append(("e10 inside", f"M1 2L{hi} 3", P))
    zeros30 = "0." + "0" * 30
    out += [("30 leading zeros", f"M{zeros30}123 1L-{zeros30}1234567890123456789 2", P),
            ("30 leading zeros", f"M1 2l.{'0' * 30}5e31 {zeros30}25E+32", P),
            ("25 trailing zeros", f"M7{'0' * 25}e-25 1L1234567890123456789{'0' * 25}e-40 2", P),
            ("25 trailing zeros", f"M1 2L5{'0' * 25}.000e-24 -12{'0' * 25}e-26", P),
            ("zero", "M0e999 -0.000e-999L0.0e-999 -0E+999", P), ("zero", "M1 1l0e999 -0.000e-999", P),
            ("zero", "0e999,-0.000e-999 1,1 -0e5,2", R.KIND_POLYGON),
            ("arc flags", "M0 0A5 5 30 1.0000000000000000 0.99999999999999999 10 10", P),
            ("arc flags", "M0 0a5.0000000000000001 5 30.000000000000004 1.9999999999999998 0.10000000000000001 10 10", P),
            ("arc flags", "M0 0a1 2 3 1e-30 10000000000000000e-16 4 5", P),
            ("25 digits", "M1 2l1234567890123456789012345 1", P), ("20 digits", "M1.2345678901234567891 2L3 4", P)]
    for _ in range(8):                                          # h / v / relative chains: float32 sums of long numbers
        a = [long_form(rng.uniform(-30, 30)) for _ in range(40)]
        s = "m" + " ".join(a[:2])
        for i in range(2, 38, 3):
            s += "h" + a[i] + "v" + a[i + 1] + "l" + a[i + 2] + ("" if a[i + 3][0] == "-" else " ") + a[i + 3]
        out.append(("relative chain", s, P))
    return out


def main():
    none = (np.zeros(0, np.int8), np.zeros((0, 11), np.float32))
    entries = []
    for tag, s, kind in slow_of_parse_npz() + grammar_strings():
        flag, cmd, args = G.reference(s, kind)
        if not inside(s, kind):
            assert flag == ROWS, (tag, s)                          # the reference reads it; the exact rule does not
            flag, cmd, args = (SLOW,) + none
        assert np.isfinite(args).all(), (tag, s)
        entries.append((tag, s, kind, flag, cmd, args))
    raw = [e[1].encode("utf-8") for e in entries]
    out = {
        "data": np.frombuffer(b"".join(raw), dtype=np.uint8),
        "offsets": np.cumsum([0] + [len(r) for r in raw]).astype(np.int64),
        "kind": np.array([e[2] for e in entries], dtype=np.uint8),
        "flag": np.array([e[3] for e in entries], dtype=np.uint8),
        "tag": np.array([e[0] for e in entries]),
        "row_offsets": np.cumsum([0] + [len(e[4]) for e in entries]).astype(np.int64),
        "commands": np.concatenate([e[4] for e in entries]),
        "args": np.concatenate([e[5] for e in entries]),
    }
    path = os.path.join(HERE, "svgio", "exact.npz")
    np.savez_compressed(path, **out)
    flags = out["flag"]
    fast = sum(G.fast(e[1], e[2]) for e in entries)
    print(f"{len(entries)} strings ({sum(len(r) for r in raw)} bytes, {len(out['commands'])} rows, at most "
          f"{int(np.diff(out['row_offsets']).max())} per string): {(flags == ROWS).sum()} with rows, {(flags == RAISES).sum()} raise, "
          f"{(flags == EMPTY).sum()} empty, {(flags == SLOW).sum()} outside the exact domain; {fast} inside the fast rule; "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
