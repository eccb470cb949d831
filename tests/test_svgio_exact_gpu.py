"""The exact number rule on the device: dsvg_svg_parse_exact against its restatement (tests/svgio_exact_ref.py) by bits - on the
reference's rows (tests/golden/svgio/exact.npz, parse.npz), on long tokens across a tile boundary at every offset, on tiles
that mix numbers of both rules, on more workgroups than the chip holds at once, on the order of errors - and `load_svgs` with
`numbers="exact"` on documents printed the way the reference's save_svg prints them."""
import itertools

import numpy as np
import pytest
import torch

from deepsvg_amd import svgio
from tests import svgio_exact_ref as X
from tests import svgio_ref as R
from tests.test_svgio_exact_host import GOLD, GOLD_EXACT, ROWS, SLOW, generic_batch, saved_documents, strings_of

pytestmark = pytest.mark.gpu
T = R.TILE
KEYS = ("commands", "args", "len_groups", "status", "valid")
# inside the fast rule, and outside it: 17 digits, 2^53 + 1, 19 digits, 1e23, 1.5e-30 (the long division), a float32 through
# repr(); the last three stay SLOW_NUMBER under the exact rule too (20 digits, a decimal exponent of 39, 25 digits)
FAST = [b"1.5", b"-7.25", b"3e2", b"12345.6789"]
LONG = [b"0.12345678901234567", b"9007199254740993", b"1234567890123456789", b"1e23", b"1.5e-30", b"-5.9604644775390625e-08"]
STAY = [b"12345678901234567891", b"1e39", b"1234567890123456789012345"]


def run(strings, kind, slot, N, G, S, numbers="exact"):
    """the kernel and the restatement on the same packed strings -> (device result as numpy, expected)"""
    data, off = svgio.pack_strings(strings)
    kind = np.zeros(len(strings), np.uint8) if kind is None else np.asarray(kind, np.uint8)
    slot = np.asarray(slot, np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    res = svgio.parse_paths(dev(data), dev(off), dev(kind), dev(slot), N=N, G=G, S=S, numbers=numbers)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}, X.parse_paths(data, off, kind, slot, N, G, S, numbers=numbers)


def same(got, exp, what=""):
    for k in KEYS:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        if k == "args":
            assert np.array_equal(R.bits(got[k]), R.bits(exp[k])), (what, k, np.argwhere(R.bits(got[k]) != R.bits(exp[k]))[:4])
        else:
            assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:4])


def test_exact_entry_equals_the_restatement_and_the_reference_on_exact_npz_in_one_launch():
    gold = dict(np.load(GOLD_EXACT))
    strings = strings_of(gold)
    P = len(strings)
    got, exp = run(strings, gold["kind"], np.arange(P), N=P, G=1, S=64)
    same(got, exp)
    assert np.array_equal(got["status"], np.where(gold["flag"] == SLOW, R.SLOW_NUMBER, R.OK)) and (gold["flag"] == ROWS).sum() >= 140
    assert (got["len_groups"].reshape(-1) == np.diff(gold["row_offsets"])).all()
    for p in np.flatnonzero(gold["flag"] == ROWS):                      # the reference's own rows, without the restatement between
        lo, hi = gold["row_offsets"][p], gold["row_offsets"][p + 1]
        assert np.array_equal(got["commands"][p, 0, 1:1 + hi - lo], gold["commands"][lo:hi].astype(np.float32)), gold["tag"][p]
        assert np.array_equal(R.bits(got["args"][p, 0, 1:1 + hi - lo]), R.bits(gold["args"][lo:hi])), gold["tag"][p]


def test_both_entries_on_parse_npz():
    gold = dict(np.load(GOLD))
    strings, flags = strings_of(gold), gold["flag"]
    P = len(strings)
    got, exp = run(strings, gold["kind"], np.arange(P), N=P, G=1, S=512)
    same(got, exp)
    slow = np.flatnonzero(flags == SLOW)
    named = [p for p in slow if gold["tag"][p] == "slow: 25 digits"]
    assert len(slow) == 31 and len(named) == 1 and got["status"][named[0]] == R.SLOW_NUMBER
    assert (got["status"][slow] == R.OK).sum() == 30 and (got["len_groups"].reshape(-1)[slow] > 0).sum() == 30
    want = np.array([R.OK, R.ARG_COUNT, R.EMPTY, R.SLOW_NUMBER])[flags]
    rest = flags != SLOW
    assert np.array_equal(got["status"][rest], want[rest])
    # flags 0..2: the two entries give identical bits
    quick, exp_quick = run(strings, gold["kind"], np.arange(P), N=P, G=1, S=512, numbers="fast")
    same(quick, exp_quick)
    assert np.array_equal(quick["status"], want)
    for k in ("commands", "len_groups", "status"):
        assert np.array_equal(got[k][rest], quick[k][rest]), k
    assert np.array_equal(R.bits(got["args"][rest]), R.bits(quick["args"][rest]))


@pytest.mark.parametrize("kind", [R.KIND_PATH, R.KIND_POLYGON])
def test_every_long_token_across_a_tile_boundary_at_every_offset(kind):
    # 12345678901234567890 has 19 significant digits and a trailing zero: by the rule it converts (w of 19 digits, e10 = 1)
    tokens = LONG + [b"12345678901234567890"] + STAY[:2]
    strings = []
    for tok in tokens:
        for boundary in (T, 2 * T):
            for inside in range(0, len(tok) + 1):            # the boundary falls in front of byte `inside` of the token
                head = b"M1 2L" if kind == R.KIND_PATH else b"1 2 "
                pad = boundary - inside - len(head)
                strings.append(head + b" " * pad + tok + b" 5 6 7")
    got, exp = run(strings, [kind] * len(strings), np.arange(len(strings)), len(strings), 1, 8)
    same(got, exp)
    per = np.cumsum([0] + [2 * (len(t) + 1) for t in tokens])
    for i, tok in enumerate(tokens):                         # one number wherever the boundary falls: it converts, or stays slow
        assert (got["status"][per[i]:per[i + 1]] == (R.SLOW_NUMBER if tok in STAY else R.OK)).all(), tok
    quick, exp_quick = run(strings, [kind] * len(strings), np.arange(len(strings)), len(strings), 1, 8, numbers="fast")
    same(quick, exp_quick)
    assert (quick["status"] == R.SLOW_NUMBER).sum() > (got["status"] == R.SLOW_NUMBER).sum()


def test_divergence_and_carry():
    pool = [FAST[0], LONG[0], LONG[4], FAST[1]]
    strings = [b"M" + b" ".join(order) for order in itertools.permutations(pool)]                      # one tile, every order
    strings += [b"M" + b" ".join(pick) + b" 1 2" for pick in itertools.product([FAST[2], LONG[1], LONG[5], STAY[0]], repeat=2)]
    assert max(map(len, strings)) <= T
    seventy = [LONG[i % len(LONG)] for i in range(70)]
    strings += [b"M" + b" ".join(seventy), b"M" + b" ".join(seventy[:69]), b"m0 0l" + b" ".join(LONG[:3] * 22 + LONG[:2] * 37)]
    strings += [LONG[0], b"M" + LONG[2], LONG[3] + b" " + LONG[5] + b" 1," + LONG[4]]                  # a single number
    kind = [0] * (len(strings) - 1) + [R.KIND_POLYLINE]
    got, exp = run(strings, kind, np.arange(len(strings)), len(strings), 1, 80)
    same(got, exp)
    assert got["len_groups"].reshape(-1)[-6:].tolist() == [35, 0, 71, 0, 0, 2]      # 70 lines and the move: the row buffer is flushed
    assert got["status"][-6:].tolist() == [R.OK, R.ARG_COUNT, R.OK, R.EMPTY, R.ARG_COUNT, R.OK]
    one, exp_one = run([b"M" + b" ".join(seventy)], None, [0], 1, 1, 40)                               # P = 1
    same(one, exp_one, "P = 1")
    assert one["status"].tolist() == [R.OK] and one["len_groups"].tolist() == [[35]]


def test_more_strings_than_the_chip_holds_at_once_with_the_smallest_groups():
    a, b, c = LONG[0], LONG[2], LONG[5]
    pool = [b"M1 2L3 4", b"M" + a + b" " + b + b"l" + c + b" 4z", b"", b"M" + a, b"M1 2L" + STAY[0] + b" 3", b"M0 0h" + c + b"v1h-1",
            b"M1 2L3 4L5 " + STAY[1], b"m.5.5 " + b + b" 1", b"L" + a + b" 1", b"#!", b"M1 2L" + LONG[3] + b" " + LONG[4]]
    P = 2 * 257 + 3
    strings = [pool[(p * 7) % len(pool)] for p in range(P)]
    got, exp = run(strings, None, np.arange(P), (P + 1) // 2, 2, 4)
    same(got, exp)
    assert {R.OK, R.EMPTY, R.ARG_COUNT, R.ROWS_OVERFLOW, R.SLOW_NUMBER} <= set(got["status"].tolist())


def test_the_first_error_in_reading_order():
    slow, long = STAY[0], LONG[0]
    strings = [b"M1 L 1 " + slow, b"M1 " + slow + b" L", b"M1 L 1 " + long, b"M1 " + long + b" L", slow + b" M1 2L3 4",
               b"1e999 " + long + b" M1 2L3 " + long, b"M1 2z" + slow, b"M1 2L" + slow + b" 3 4", b"M" + long + b" 2L3 4 5", b"M1 2z" + long]
    got, exp = run(strings, None, np.arange(len(strings)), len(strings), 1, 6)
    same(got, exp)
    assert got["status"].tolist() == [R.ARG_COUNT, R.SLOW_NUMBER, R.ARG_COUNT, R.ARG_COUNT, R.OK, R.OK, R.SLOW_NUMBER, R.SLOW_NUMBER,
                                      R.ARG_COUNT, R.ARG_COUNT]        # behind a z the number is read before it is counted


def test_load_svgs_reads_saved_float32_text_bit_for_bit_with_exact_numbers():
    cmd, args = generic_batch(8)
    docs = saved_documents(cmd, args)
    res = svgio.load_svgs(docs, max_num_groups=8, max_seq_len=30, numbers="exact")
    assert res["valid"].all() and torch.equal(res["commands"].cpu(), cmd)
    assert np.array_equal(R.bits(res["args"].cpu().numpy()), R.bits(args.numpy()))
    quick = svgio.load_svgs(docs, max_num_groups=8, max_seq_len=30)
    strings = [d.encode() for doc in docs for d in __import__("re").findall(r' d="([^"]*)"', doc)]
    slow = np.array([R.parse(s)[0] == R.SLOW_NUMBER for s in strings])
    assert np.array_equal(quick["status"].cpu().numpy() == R.SLOW_NUMBER, slow) and slow.sum() >= 8
    icon = np.repeat(np.arange(8), [doc.count("<path") for doc in docs])
    assert quick["valid"].cpu().tolist() == [not slow[icon == n].any() for n in range(8)] and not quick["valid"].all()
