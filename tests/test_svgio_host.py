"""deepsvg_amd.svgio without a GPU: the restatement (tests/svgio_ref.py) against the reference's own results
(tests/golden/svgio/parse.npz), its number pattern against `re`, its decimal rule against float(), `to_svg` read back through the
restatement, and the Python surface (`load_svgs`, `preprocess`, the meta table) against a fake `ops` that runs the restatement
on what the wrappers hand to the kernel."""
import os
import re

import numpy as np
import pytest
import torch

import deepsvg_amd
from deepsvg_amd import lib, paths, svgio
from deepsvg_amd.synthetic import make_batch
from tests import svgio_ref as R

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svgio", "parse.npz")
ROWS, RAISES, EMPTY, SLOW = range(4)                 # the flags of the golden file
FLOAT_RE = re.compile(rb"[-+]?[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def strings_of(gold):
    data = gold["data"].tobytes()
    return [data[gold["offsets"][p]:gold["offsets"][p + 1]] for p in range(len(gold["kind"]))]


def documents_of(gold):
    data = gold["doc_data"].tobytes()
    return [data[gold["doc_offsets"][i]:gold["doc_offsets"][i + 1]].decode("utf-8") for i in range(len(gold["doc_offsets"]) - 1)]


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_on_every_golden_string(gold):
    flags, tags = gold["flag"], gold["tag"]
    assert len(flags) >= 150 and (flags == RAISES).sum() >= 10 and (flags == EMPTY).sum() >= 8
    # outside the fast path: the five named strings and the reference's own saved files with 17-digit numbers, nothing else
    real = (tags == "docs slow").sum()
    assert (flags == SLOW).sum() == 5 + real and real >= 20 and (flags[tags == "docs slow"] == SLOW).all()
    assert sum(t.startswith("slow: ") for t in tags.tolist()) == 5 and int(gold["left_out_long"]) == 0
    assert {"docs", "relative chain", "M M", "M1 1z", "empty", "separators", "non-ascii", "junk"} <= set(tags.tolist())
    for p, s in enumerate(strings_of(gold)):
        st, cmd, args = R.parse(s, int(gold["kind"][p]))
        lo, hi = gold["row_offsets"][p], gold["row_offsets"][p + 1]
        what = (p, tags[p], s[:60])
        if flags[p] == ROWS:
            assert st == R.OK and np.array_equal(cmd, gold["commands"][lo:hi]), what
            assert np.array_equal(R.bits(args), R.bits(gold["args"][lo:hi])), what
        else:
            assert st == {RAISES: R.ARG_COUNT, EMPTY: R.EMPTY, SLOW: R.SLOW_NUMBER}[int(flags[p])] and len(cmd) == 0, what


def test_number_pattern_is_findall_on_seeded_strings():
    rng = np.random.RandomState(7)
    alphabet = b"0123456789" * 2 + b"..--++eE ,xM"
    cases = [b"1.5.5", b"10-2e1", b"1.", b"4e", b"4e+", b"4e+.5", b"-", b"+-.5", b"1e5.5", b"1..5", b"-.e5", b".", b"", b"5"]
    cases += [bytes(alphabet[i] for i in rng.randint(0, len(alphabet), rng.randint(1, 40))) for _ in range(20000)]
    for s in cases:
        got = [s[t[1]:t[2]] for t in R.tokens(s, R.KIND_POLYLINE)]
        assert got == FLOAT_RE.findall(s), s
    assert [t for t in R.tokens(b"1.5.5 10-2e1", R.KIND_POLYLINE)] == [("n", 0, 3), ("n", 3, 5), ("n", 6, 8), ("n", 8, 12)]
    assert R.tokens(b"3M4e", R.KIND_PATH) == [("n", 0, 1), ("c", "M"), ("n", 2, 3)]       # `e` is skipped, M is a letter


def test_decimal_rule_equals_float_on_100k_seeded_decimals():
    rng = np.random.RandomState(11)
    n = 100000
    digits = rng.randint(1, 16, n)
    for i in range(n):
        w = "".join(str(d) for d in rng.randint(0, 10, digits[i]))
        cut = rng.randint(0, len(w) + 1)
        text = w[:cut] + "." + w[cut:] if rng.randint(0, 3) else w
        if text.endswith(".") or text == "":
            text += "0"
        if rng.randint(0, 4) == 0:
            text += "e%+d" % rng.randint(-8, 9)
        text = ["", "-", "+"][rng.randint(0, 3)] + text
        v = R.decimal(text.encode())
        if v is not None:
            assert R.f64_bits(v) == R.f64_bits(float(text)), text
        else:                                        # only through the exponent: 15 digits always fit
            assert "e" in text, text
    assert R.f64_bits(R.decimal(b"-0")) == R.f64_bits(-0.0) and R.decimal(b"1e22") == 1e22 and R.decimal(b"1e23") is None
    assert R.decimal(b"9007199254740991") == 2.0 ** 53 - 1 and R.decimal(b"9007199254740992") is None
    assert R.decimal(b"0.000000000000000000000000000001000") is None and R.decimal(b"000.5000") == 0.5
    assert R.decimal(b"1" + b"0" * 30) is None and R.decimal(b"0" * 40 + b"7") == 7.0


def test_status_rules():
    assert R.parse(b"M0 0" + b"l1 1" * 5, S=8)[0] == R.OK and R.parse(b"M0 0" + b"l1 1" * 5, S=7)[0] == R.ROWS_OVERFLOW    # six rows
    big = b"9000000000000000e22"                                                          # 9e37: the largest the fast path reads
    assert R.parse(b"M" + big + b" 0l" + (big + b" 0 ") * 2)[0] == R.OK
    assert R.parse(b"M" + big + b" 0l" + (big + b" 0 ") * 3)[0] == R.RANGE                 # the fourth float32 sum overflows
    assert R.parse(b"M1 2L")[0] == R.ARG_COUNT and R.parse(b"M1 2L3 1e23")[0] == R.SLOW_NUMBER
    assert R.parse(b"M1 1e23 L")[0] == R.SLOW_NUMBER and R.parse(b"M1 L 1e23 1")[0] == R.ARG_COUNT   # the first in reading order
    assert R.parse(b"1e999 M1 2L3 4")[0] == R.OK                                          # never converted
    data, off = svgio.pack_strings([b"M1 1l1 1", b"M2 2l1 1", b"M3 3l1 1", b"M4 4l1 1", b"M1"])
    res = R.parse_paths(data, off, np.zeros(5, np.uint8), np.array([0, 0, 5, -1, 2], np.int32), 2, 2, 4)
    assert res["status"].tolist() == [R.BAD_SLOT, R.BAD_SLOT, R.BAD_SLOT, R.OK, R.ARG_COUNT]
    assert res["valid"].tolist() == [False, False] and (res["commands"][:, :, 1:] == R.EOS).all() and (res["args"] == -1).all()


# ---- to_svg ---------------------------------------------------------------------------------------------------------------------------
def test_to_svg_reads_back_bit_for_bit_through_the_restatement():
    rng = np.random.RandomState(3)
    values = np.concatenate([np.arange(256), np.arange(-2048, 2048) / 8.0, rng.uniform(-1e4, 1e4, 100000),
                             rng.uniform(-1, 1, 2000) * 10.0 ** rng.randint(-12, 13, 2000), [0.0, -0.0]]).astype(F)
    values = values[: len(values) // 2 * 2]
    n = len(values) // 2
    G, S = 4, 1 + 2046 // 4
    rows = G * (S - 2)
    N = -(-n // rows)
    cmd = np.full((N, G, S), R.EOS, dtype=F)
    cmd[:, :, 0] = R.SOS
    args = np.full((N, G, S, 11), -1.0, dtype=F)
    flat_c, flat_a = cmd[:, :, 1:S - 1].reshape(-1), args[:, :, 1:S - 1].reshape(-1, 11)
    flat_c[:n] = R.L
    flat_a[:n, 9:] = values.reshape(n, 2)
    cmd[:, :, 1:S - 1], args[:, :, 1:S - 1] = flat_c.reshape(N, G, S - 2), flat_a.reshape(N, G, S - 2, 11)
    cmd[:, :, 1] = np.where(cmd[:, :, 1] == R.L, R.M, cmd[:, :, 1])
    docs = svgio.to_svg(torch.from_numpy(cmd), torch.from_numpy(args))
    assert len(docs) == N
    for i, doc in enumerate(docs):
        ds = re.findall(r' d="([^"]*)"', doc)
        for g, d in enumerate(ds):
            st, c, a = R.parse(d.encode(), R.KIND_PATH, S)
            k = len(c)
            assert st == (R.OK if k else R.EMPTY) and np.array_equal(c, cmd[i, g, 1:1 + k]) and cmd[i, g, 1 + k] == R.EOS
            assert np.array_equal(R.bits(a), R.bits(args[i, g, 1:1 + k])), (i, g)
    assert 'filling="0"' in docs[0] and 'viewBox="0 0 256 256"' in docs[0] and " d=\"M" in docs[0]


def test_to_svg_letters_arcs_and_refusals():
    cmd, args = np.full((1, 2, 6), R.EOS, dtype=F), np.full((1, 2, 6, 11), -1.0, dtype=F)
    cmd[0, :, 0] = R.SOS
    cmd[0, 1, 1:5] = [R.M, R.C, R.A, R.Z]
    args[0, 1, 1, 9:], args[0, 1, 2, 5:] = (1.5, -2), (1, 2, 3, 4, 5, 0.1)
    args[0, 1, 3, :5], args[0, 1, 3, 9:] = (3, 4, 30, 0, 1), (7, 8)
    doc, = svgio.to_svg(cmd, args, filling=np.array([[0, 2]]), viewbox=24)
    assert doc == ('<svg xmlns="http://www.w3.org/2000/svg" viewBox="0 0 24 24"><path fill="none" filling="0" d=""/>'
                   '<path fill="none" filling="2" d="M1.5 -2 C1 2 3 4 5 0.1 A3 4 30 0 1 7 8 Z"/></svg>')
    for bad in (np.inf, np.nan, 1e30):
        args[0, 1, 1, 9] = bad
        with pytest.raises(ValueError):
            svgio.to_svg(cmd, args)
    args[0, 1, 1, 9] = 1.0
    cmd[0, 1, 2] = R.SOS
    with pytest.raises(ValueError):
        svgio.to_svg(cmd, args)
    with pytest.raises(ValueError):
        svgio.to_svg(cmd, args[:, :, :5])


# ---- the Python surface, against a fake ops that runs the restatement ------------------------------------------------------------------
class _FakeOps:
    def __init__(self):
        self.calls = []

    def require_device(self, device):
        pass

    def svg_parse(self, data, offsets, kind, slot, N, G, S):
        self.calls.append((data, offsets, kind, slot, N, G, S))
        assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and kind.dtype == torch.uint8 and slot.dtype == torch.int32
        assert all(t.is_contiguous() and t.dim() == 1 for t in (data, offsets, kind, slot))
        res = R.parse_paths(data.numpy(), offsets.numpy(), kind.numpy(), slot.numpy(), N, G, S)
        return {k: torch.from_numpy(v) for k, v in res.items()}


@pytest.fixture
def fake_ops(monkeypatch):
    fake = _FakeOps()
    monkeypatch.setattr(svgio, "ops", fake)
    return fake


def check_documents(gold, res, G):
    go, ro = gold["doc_group_offsets"], gold["doc_row_offsets"]
    cmd, args, lens = res["commands"].cpu().numpy(), res["args"].cpu().numpy(), res["len_groups"].cpu().numpy()
    assert res["valid"].cpu().all() and np.array_equal(R.bits(res["viewbox"].cpu().numpy()), R.bits(gold["doc_viewbox"]))
    for n in range(len(go) - 1):
        k = go[n + 1] - go[n]
        assert k <= G and (lens[n, k:] == 0).all() and (cmd[n, k:, 1:] == R.EOS).all()
        assert res["fill"][n, :k].tolist() == gold["doc_fill"][go[n]:go[n + 1]].tolist()
        assert res["filling"][n, :k].tolist() == gold["doc_filling"][go[n]:go[n + 1]].tolist()
        assert (res["source"][n, :k] >= 0).all() and (res["source"][n, k:] == -1).all()
        for g in range(k):
            lo, hi = ro[go[n] + g], ro[go[n] + g + 1]
            assert lens[n, g] == hi - lo and cmd[n, g, 0] == R.SOS and (cmd[n, g, 1 + hi - lo:] == R.EOS).all(), (n, g)
            assert np.array_equal(cmd[n, g, 1:1 + hi - lo], gold["doc_commands"][lo:hi].astype(F)), (n, g)
            assert np.array_equal(R.bits(args[n, g, 1:1 + hi - lo]), R.bits(gold["doc_args"][lo:hi])), (n, g)
            assert (args[n, g, 0] == -1).all() and (args[n, g, 1 + hi - lo:] == -1).all()


def test_load_svgs_equals_the_reference_on_the_six_documents(gold, fake_ops):
    docs = documents_of(gold)
    assert len(docs) == 6
    res = svgio.load_svgs(docs, max_num_groups=6, max_seq_len=10, device="cpu")
    check_documents(gold, res, 6)
    assert len(fake_ops.calls) == 1                                   # one call for the whole list
    assert res["source"][2].tolist() == [0, 2, 1, 3, -1, -1]          # paths first, then the rect, then the circle


def test_load_svgs_drops_icons_not_batches(gold, fake_ops):
    good = documents_of(gold)[0]
    docs = [good, "<svg viewBox='0 0 1 1'><path d='M1 2L3'/></svg>", "not xml", "<svg viewBox='0 0 1'><path d='M1 2L3 4'/></svg>",
            "<svg viewBox='0 0 1 1'>" + "<path d='M1 2L3 4'/>" * 3 + "</svg>", "<svg viewBox='0,0, 2 2'><rect width='x' height='1'/></svg>",
            "<svg viewBox='0,0, 2 2'><circle cx='1' cy='1' r='1'/></svg>", "<svg viewBox='0 0 1 1'><rect width='1' height='1'/><path d='M1'/></svg>"]
    res = svgio.load_svgs(docs, max_num_groups=2, max_seq_len=6, device="cpu")
    assert res["valid"].tolist() == [True, False, False, False, False, False, True, False]
    bad = ~res["valid"]
    assert (res["commands"][bad][:, :, 1:] == R.EOS).all() and (res["args"][bad] == -1).all() and (res["len_groups"][bad] == 0).all()
    assert res["len_groups"][0].tolist() == [4, 4] and res["len_groups"][6].tolist() == [6, 0]
    assert res["viewbox"][6].tolist() == [0, 0, 2, 2]
    small = svgio.load_svgs(docs[6:7], max_num_groups=1, max_seq_len=5, device="cpu")          # six rows do not fit five
    assert small["valid"].tolist() == [False]
    with pytest.raises(ValueError):
        svgio.load_svgs([], 2, 6, "cpu")
    with pytest.raises(ValueError):
        svgio.load_svgs(docs, 2, 2046, "cpu")


def test_parse_paths_packs_strings_and_refuses_bad_arguments(fake_ops):
    res = svgio.parse_paths(["M1 2L3 4", "M5 6h1", "1,2 3,4"], icon=[1, 0, 1], kind=[0, 0, 2], G=2, S=6, device="cpu")
    data, offsets, kind, slot, N, G, S = fake_ops.calls[0]
    assert bytes(data.numpy()) == b"M1 2L3 4M5 6h11,2 3,4" and offsets.tolist() == [0, 8, 14, 21]
    assert slot.tolist() == [2, 0, 3] and kind.tolist() == [0, 0, 2] and (N, G, S) == (2, 2, 6)
    assert res["len_groups"].tolist() == [[2, 0], [2, 3]] and res["status"].tolist() == [0, 0, 0]
    over = svgio.parse_paths(["M1 2L3 4"] * 3, G=2, S=6, device="cpu")
    assert over["status"].tolist() == [R.OK, R.OK, R.BAD_SLOT]
    t = lambda a, dt: torch.tensor(a, dtype=dt)                       # noqa: E731
    good = (t([77, 49], torch.uint8), t([0, 2], torch.int64), t([0], torch.uint8), t([0], torch.int32))
    assert svgio.parse_paths(*good, N=1, G=1, S=4)["status"].tolist() == [R.ARG_COUNT]
    for bad in ((good[0].int(),) + good[1:], good[:1] + (good[1].int(),) + good[2:], good[:3] + (t([0, 0], torch.int32),)):
        with pytest.raises(ValueError):
            svgio.parse_paths(*bad, N=1, G=1, S=4)
    for shape in ((0, 1, 4), (1, 0, 4), (1, 1, 1), (1, 2, 1025), (1, 1, 4.0)):
        with pytest.raises(ValueError):
            svgio.parse_paths(*good, N=shape[0], G=shape[1], S=shape[2])
    with pytest.raises(ValueError):
        svgio.parse_paths(["M1 2"], offsets=good[1], G=1, S=4)
    with pytest.raises(ValueError):
        svgio.parse_paths([], G=1, S=4)
    with pytest.raises(ValueError):
        svgio.parse_paths(*good)


def test_preprocess_composes_the_chain_of_paths(monkeypatch):
    calls = []
    N, G, S = 3, 2, 6
    cmd, args = torch.zeros(N, G, S), torch.zeros(N, G, S, 11)

    def link(name, **extra):
        def run(c, a, *pos, **kw):
            calls.append((name, pos, kw))
            n, g = c.shape[0], kw.get("max_num_groups", c.shape[1])
            s = (kw["max_seq_len"] + 2) if kw.get("max_seq_len") is not None else c.shape[2]
            out = {"commands": torch.zeros(n, g, s), "args": torch.zeros(n, g, s, 11), "valid": torch.ones(n, dtype=torch.bool),
                   "len_groups": torch.full((n, g), 3, dtype=torch.int32)}
            out.update(extra)
            return out
        return run

    monkeypatch.setattr(paths, "arcs_to_beziers", link("arcs"))
    monkeypatch.setattr(paths, "transform", link("transform"))
    src = torch.tensor([[1, 0, -1], [0, -1, -1], [1, 1, 0]], dtype=torch.int32)
    monkeypatch.setattr(paths, "canonicalize", link("canon", source_group=src, valid=torch.tensor([True, False, True])))
    monkeypatch.setattr(paths, "simplify_heuristic", link("simplify"))
    vb = torch.tensor([[0, 0, 24, 24], [10, 20, 100, 50], [-1, -2, 3, 0.7]], dtype=torch.float32)
    batch = {"commands": cmd, "args": args, "viewbox": vb, "valid": torch.tensor([True, True, False]),
             "filling": torch.tensor([[1, 2], [2, 0], [0, 1]], dtype=torch.int32)}
    res = svgio.preprocess(batch, max_num_groups=3, max_seq_len=8)
    assert [c[0] for c in calls] == ["arcs", "transform", "canon", "simplify"]
    work = 2048 // 3 - 2
    assert calls[0][2] == {"max_seq_len": work} and calls[2][2] == {"max_num_groups": 3, "max_seq_len": work}
    assert calls[3][2] == {"unit": 1.0, "max_seq_len": 8, "work_seq_len": work}
    steps = calls[1][1][0]
    assert [s[0] for s in steps] == ["translate", "scale", "translate", "translate", "scale", "translate"]
    v = vb.numpy()
    centre = v[:, :2] + v[:, 2:] * F(0.5)
    assert np.array_equal(R.bits(steps[0][1].numpy()), R.bits(-centre))                      # float32, as _normalize_steps forms it
    assert np.array_equal(R.bits(steps[1][1].numpy()), R.bits(F(24) / v[:, 2:].max(axis=1)))
    assert tuple(steps[2][1]) == (12.0, 12.0) and steps[4][1] == 0.9
    assert np.array_equal(steps[3][1], np.array([-12, -12], F)) and np.array_equal(steps[5][1], np.array([12, 12], F))
    assert res["valid"].tolist() == [True, False, False] and res["filling"].tolist() == [[2, 1, 0], [2, 0, 0], [1, 1, 0]]
    assert res["len_groups"].tolist() == [[3, 3, 3], [0, 0, 0], [0, 0, 0]] and res["n_groups"].tolist() == [3, 0, 0]
    assert res["commands"].shape == (3, 3, 10)
    for bad in ({"max_num_groups": 0}, {"max_seq_len": -1}, {"max_num_groups": 64, "max_seq_len": 31}, {"work_seq_len": 2000}):
        with pytest.raises(ValueError):
            svgio.preprocess(batch, **bad)
    with pytest.raises(ValueError):
        svgio.preprocess({**batch, "viewbox": vb[:, :3]})


def test_meta_table_is_the_reference_s_and_filter_meta_takes_it():
    from deepsvg_amd.dataset import SVGTensorDataset
    lens = torch.tensor([[4, 7, 0, 0], [31, 2, 2, 0], [3, 0, 0, 0], [5, 5, 5, 5]], dtype=torch.int32)
    df = svgio.meta_table(["a", "b", "c", "d"], lens)
    assert list(df.columns) == ["id", "total_len", "nb_groups", "len_groups", "max_len_group"]
    assert df.total_len.tolist() == [11, 35, 3, 20] and df.nb_groups.tolist() == [2, 3, 1, 4]
    assert df.len_groups.tolist() == [[4, 7], [31, 2, 2], [3], [5, 5, 5, 5]] and df.max_len_group.tolist() == [7, 31, 3, 5]
    assert SVGTensorDataset.filter_meta(df, 3, 30).id.tolist() == ["a", "c"]
    assert SVGTensorDataset.filter_meta(df, 8, 30, max_total_len=11).id.tolist() == ["a", "c"]
    with pytest.raises(ValueError):
        svgio.meta_table(["a"], lens)


def test_binding_matches_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsvg.h")).read()
    decl = re.search(r"int dsvg_svg_parse\(([^)]*)\);", hdr).group(1)
    assert len(lib.SIGNATURES["dsvg_svg_parse"][1]) == len(decl.split(",")) == 16
    assert lib.ABI_VERSION == int(re.search(r"#define DSVG_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("PATH", "POLYLINE", "POLYGON", "OK", "EMPTY", "ARG_COUNT", "SLOW_NUMBER", "ROWS_OVERFLOW", "BAD_SLOT", "RANGE", "TILE"):
        assert getattr(lib, "DSVG_SVG_" + name) == int(re.search(r"#define DSVG_SVG_%s (\d+)" % name, hdr).group(1)), name
    assert svgio.STATUS[R.RANGE] == "RANGE" and svgio.TILE == R.TILE and "svgio" in deepsvg_amd.__all__
    src = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "build.sh")).read()
    assert " svg_parse" in src


def test_to_svg_then_load_svgs_is_the_identity_on_a_synthetic_batch(fake_ops):
    cmd, args = make_batch(8, seed=5)
    res = svgio.load_svgs(svgio.to_svg(cmd, args), max_num_groups=8, max_seq_len=30, device="cpu")
    assert res["valid"].all() and torch.equal(res["commands"], cmd) and torch.equal(res["args"], args)
