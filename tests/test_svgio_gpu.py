"""deepsvg_amd.svgio on the device: csrc/svg_parse.hip against the restatement (tests/svgio_ref.py) by bits - on the reference's
golden strings and on the smallest shapes at which the kernel can still go wrong: the tile size and its neighbours, every token
kind across a tile boundary at every offset, more workgroups than the chip holds at once, the row bound, the slot rules -
and the layers above it: `load_svgs` against the reference's documents, `preprocess_files` against the same chain called by
hand, `to_svg -> load_svgs` as the identity."""
import numpy as np
import pytest
import torch

from deepsvg_amd import paths, svgio
from deepsvg_amd.synthetic import make_batch
from tests import poison
from tests import svgio_ref as R
from tests.test_svgio_host import GOLD, check_documents, documents_of, strings_of

pytestmark = pytest.mark.gpu
F = np.float32
T = R.TILE
KEYS = ("commands", "args", "len_groups", "status", "valid")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def run(strings, kind, slot, N, G, S):
    """the kernel and the restatement on the same packed strings -> (device result as numpy, expected)"""
    data, off = svgio.pack_strings(strings)
    kind = np.zeros(len(strings), np.uint8) if kind is None else np.asarray(kind, np.uint8)
    slot = np.asarray(slot, np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()       # noqa: E731
    res = svgio.parse_paths(dev(data), dev(off), dev(kind), dev(slot), N=N, G=G, S=S)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in KEYS}, R.parse_paths(data, off, kind, slot, N, G, S)


def same(got, exp, what=""):
    for k in KEYS:
        assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
        if k == "args":
            assert np.array_equal(R.bits(got[k]), R.bits(exp[k])), (what, k, np.argwhere(R.bits(got[k]) != R.bits(exp[k]))[:4])
        else:
            assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:4])


def test_kernel_equals_the_restatement_on_the_golden_set_in_one_launch(gold):
    strings = strings_of(gold)
    P = len(strings)
    got, exp = run(strings, gold["kind"], np.arange(P), N=P, G=1, S=512)
    same(got, exp)
    # and the restatement is the reference there (tests/test_svgio_host.py): the statuses, once more, from the file's flags
    want = np.array([R.OK, R.ARG_COUNT, R.EMPTY, R.SLOW_NUMBER])[gold["flag"]]
    assert np.array_equal(got["status"], want)
    assert (got["len_groups"].reshape(-1) == np.diff(gold["row_offsets"])).all()


def test_one_string_and_the_tile_sizes():
    got, exp = run([b"M1 2L3 4"], None, [0], 1, 1, 4)
    same(got, exp, "P = 1")
    assert got["status"].tolist() == [R.OK] and got["len_groups"].tolist() == [[2]]
    strings = []
    for n in (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 5 * T):
        body = b"M1 2L3 4 5 6"
        strings += [b" " * n, b"7" * min(n, 15) + b" " * max(n - 15, 0), (body + b" " * n)[:n],
                    (b" " * n + body)[-n:] if n else b"", (b"M" + b" 1.25" * (n // 5 + 1))[:n], b"z" * n, b"M" * n]
    got, exp = run(strings, None, np.arange(len(strings)), len(strings), 1, 2 * T + 8)
    same(got, exp, "tile sizes")
    assert (np.diff(svgio.pack_strings(strings)[1])[::7] == [0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 5 * T]).all()


@pytest.mark.parametrize("kind", [R.KIND_PATH, R.KIND_POLYGON])
def test_every_token_kind_across_a_tile_boundary_at_every_offset(kind):
    tokens = [b"12345.6789", b"1.5e-12", b"-7.25", b"+.5", b"1.5.5", b"4e+.5", b"4e+-5", b"1..5", b"10-2e1", b"3e", b"3e+ ", b"2.e1",
              b"00.0100e+01", b"9007199254740993", b"1e23"]
    strings = []
    for tok in tokens:
        for boundary in (T, 2 * T):
            for inside in range(0, len(tok) + 1):            # the boundary falls in front of byte `inside` of the token
                head = b"M1 2L" if kind == R.KIND_PATH else b"1 2 "
                pad = boundary - inside - len(head)
                strings.append(head + b" " * pad + tok + b" 5 6 7")
    got, exp = run(strings, [kind] * len(strings), np.arange(len(strings)), len(strings), 1, 8)
    same(got, exp)
    assert {R.OK, R.ARG_COUNT, R.SLOW_NUMBER} <= set(got["status"].tolist())


def test_more_strings_than_the_chip_holds_at_once_with_the_smallest_groups():
    pool = [b"M1 2L3 4", b"M1 2l3 4z", b"", b"M1 2", b"M1 2L3", b"M0 0h1v1h-1", b"M1 2L3 4L5 6", b"m.5.5 1 1", b"L1 1", b"#!"]
    P = 2 * 257 + 3
    strings = [pool[(p * 7) % len(pool)] for p in range(P)]
    got, exp = run(strings, None, np.arange(P), (P + 1) // 2, 2, 4)
    same(got, exp)
    assert {R.OK, R.EMPTY, R.ARG_COUNT, R.ROWS_OVERFLOW} <= set(got["status"].tolist())


def test_the_row_bound():
    S = 70                                           # more rows than collect in LDS at once
    fit, over = b"M0 0" + b"l1 1" * (S - 3), b"M0 0" + b"l1 1" * (S - 2)
    poly = b" ".join(b"%d %d" % (i, i) for i in range(S - 3))
    strings = [fit, over, fit + b"z", b"M0 0" + b"c1 1 2 2 3 3" * (S - 3), poly, poly + b" 9 9", poly, poly + b" 9 9",
               b"M0 0" + b"l1 1" * 400, b"M1 1zl1 1" * 300 + b"M0 0l1 1"]
    kind = [0, 0, 0, 0, R.KIND_POLYGON, R.KIND_POLYGON, R.KIND_POLYLINE, R.KIND_POLYLINE, 0, 0]
    got, exp = run(strings, kind, np.arange(len(strings)), len(strings), 1, S)
    same(got, exp)
    assert got["status"].tolist() == [R.OK, R.ROWS_OVERFLOW, R.ROWS_OVERFLOW, R.OK, R.OK, R.ROWS_OVERFLOW, R.OK, R.OK,
                                      R.ROWS_OVERFLOW, R.OK]
    assert got["len_groups"].reshape(-1).tolist() == [S - 2, 0, 0, S - 2, S - 2, 0, S - 3, S - 2, 0, 2]


def test_slots_junk_and_an_invalid_icon_beside_valid_ones():
    strings = [b"M1 2L3 4", b"M5 6L7 8", b"M1 2L3 4", b"M9 9l1 1", b"M1", b"M2 2l2 2", b"\xff\xfe ;; ~~", b"M3 3l3 3", b"M4 4l4 4",
               b"M1 2L3 4", b"M6 6l6 6"]
    slot = [0, 1, 2, 2, 4, 5, 6, -1, 8, 99, -2]      # 2 is shared, 4 fails, 6 is junk (EMPTY), 99 and -2 are out of range
    got, exp = run(strings, None, slot, 5, 2, 6)
    same(got, exp)
    assert got["status"].tolist() == [R.OK, R.OK, R.BAD_SLOT, R.BAD_SLOT, R.ARG_COUNT, R.OK, R.EMPTY, R.OK, R.OK, R.BAD_SLOT,
                                      R.BAD_SLOT]
    assert got["valid"].tolist() == [True, False, False, True, True]
    assert got["len_groups"].tolist() == [[2, 2], [0, 0], [0, 0], [0, 0], [2, 0]]
    assert (got["commands"][[1, 2, 3], :, 1:] == R.EOS).all() and (got["args"][[1, 2, 3]] == -1).all()


def test_runs_are_bit_identical_and_every_output_element_is_written(gold):
    strings = strings_of(gold)[:64] + [b"M1 2L3 4", b"M1 2L3 4", b"M1"]
    P = len(strings)
    data, off = svgio.pack_strings(strings)
    slot = np.arange(P, dtype=np.int32)
    slot[-2] = slot[-3]                              # a shared slot: whichever index stays must not show
    kind = np.concatenate([gold["kind"][:64], np.zeros(3, np.uint8)])
    dev = [torch.from_numpy(a).cuda() for a in (data, off, kind, slot)]

    def once():
        res = svgio.parse_paths(*dev, N=(P + 3) // 4, G=4, S=300)
        return {k: res[k].cpu() for k in KEYS}

    runs = poison.three_runs(once) + [once()]
    exp = R.parse_paths(data, off, kind, slot, (P + 3) // 4, 4, 300)
    for r in runs:
        same({k: v.numpy() for k, v in r.items()}, exp)
        assert not torch.isnan(r["args"]).any()


def test_load_svgs_equals_the_reference_on_the_six_documents(gold):
    res = svgio.load_svgs(documents_of(gold), max_num_groups=6, max_seq_len=10)
    assert res["commands"].is_cuda and res["viewbox"].is_cuda
    check_documents(gold, {k: v.cpu() for k, v in res.items()}, 6)


def test_preprocess_files_equals_the_chain_called_by_hand(gold, tmp_path):
    docs = documents_of(gold)
    files = []
    for i, d in enumerate(docs):
        files.append(tmp_path / f"icon{i}.svg")
        files[-1].write_text(d)
    G, L = 6, 40
    store, meta = svgio.preprocess_files([str(f) for f in files], max_num_groups=G, max_seq_len=L)
    batch = svgio.load_svgs(docs, max_num_groups=G, max_seq_len=L)
    work = 2048 // G - 2
    vb = batch["viewbox"].cpu().numpy()
    kept, rows, lens = [], [], []
    for n in range(len(docs)):                       # one icon at a time, Python numbers as parameters, one call per link
        c, a = batch["commands"][n:n + 1], batch["args"][n:n + 1]
        flat = paths.arcs_to_beziers(c, a, max_seq_len=work)
        centre = vb[n, :2] + vb[n, 2:] * F(0.5)
        moved = paths.transform(flat["commands"], flat["args"],
                                [("translate", tuple(-centre)), ("scale", F(24) / vb[n, 2:].max()), ("translate", (12.0, 12.0))])
        zoomed = paths.zoom(moved["commands"], moved["args"], 0.9, viewbox=24)
        canon = paths.canonicalize(zoomed["commands"], zoomed["args"], max_num_groups=G, max_seq_len=work)
        simple = paths.simplify_heuristic(canon["commands"], canon["args"], unit=1.0, max_seq_len=L, work_seq_len=work)
        ok = bool(flat["valid"] & canon["valid"] & simple["valid"]) and int((simple["len_groups"] > 0).sum()) > 0
        if ok:
            kept.append(f"icon{n}")
            ln = simple["len_groups"][0].cpu().numpy()
            lens.append(ln)
            for g in range(G):
                rows.append(torch.cat([simple["commands"][0, g, 1:1 + ln[g], None], simple["args"][0, g, 1:1 + ln[g]]], dim=1))
    assert len(kept) >= 5 and store.ids == kept and meta.id.tolist() == kept
    want = torch.cat(rows).cpu().numpy()
    assert np.array_equal(R.bits(store.rows.cpu().numpy()), R.bits(want))
    assert store.viewbox == 24.0 and store.G == G
    assert np.array_equal(np.diff(store.slot_off.cpu().numpy()), np.concatenate(lens))
    assert meta.total_len.tolist() == [int(ln.sum()) for ln in lens]
    assert meta.nb_groups.tolist() == [int((ln > 0).sum()) for ln in lens]


def test_to_svg_then_load_svgs_is_the_identity_on_a_decoded_batch():
    cmd, args = make_batch(8, seed=5)
    res = svgio.load_svgs(svgio.to_svg(cmd.cuda(), args.cuda()), max_num_groups=8, max_seq_len=30)
    assert res["valid"].all() and torch.equal(res["commands"].cpu(), cmd)
    assert np.array_equal(R.bits(res["args"].cpu().numpy()), R.bits(args.numpy()))
