"""No-GPU check of the hand-scheduled kernels: from the gfx950 assembly hipcc cross-compiles here, no kernel of the token-
stationary files keeps a register spill inside a loop (a scratch reload there is followed by `s_waitcnt vmcnt(0)`, i.e. it
drains the weight stream's DMA every iteration)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
@pytest.mark.parametrize("src", ["ffn_fused", "attn_fused"])
def test_no_spill_inside_a_loop(tmp_path, src):
    out = tmp_path / f"{src}.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result",
                    "-Wno-unused-value", "-S", "--cuda-device-only", os.path.join(ROOT, "deepsvg_amd", "csrc", f"{src}.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_loop_mix.py"), "--spills", str(out)],
                       check=True, capture_output=True, text=True)
    rows = [l for l in r.stdout.splitlines() if "scratch instructions" in l]
    inside = [l for l in rows if int(re.search(r"inside loops\s+(\d+)", l).group(1)) > 0]
    assert not inside, "\n".join(inside)
    assert any("mfma" in l for l in r.stdout.splitlines())          # the scan found the kernels' loops


def test_committed_ffn_traffic_was_measured_on_this_kernel_source():
    """profiles/ffn_traffic.json (bench.py's roofline.traffic, a committed rocprofv3 --pmc measurement) names the code of
    csrc/ffn_fused.hip it was collected on: an edited kernel makes the number stale - re-run scripts/gpu_ffn_traffic.sh"""
    import json
    sys.path.insert(0, ROOT)
    import bench
    t = json.load(open(os.path.join(ROOT, "profiles", "ffn_traffic.json")))
    assert t["ffn_fused_hip_code_sha256_16"] == bench.kernel_source_hash(os.path.join(ROOT, "deepsvg_amd", "csrc", "ffn_fused.hip"))
    assert t.get("commit")


def _csrc_code():
    """{file name: text} of csrc/*.hip and csrc/*.h with comments removed the way bench.kernel_source_hash removes them"""
    d = os.path.join(ROOT, "deepsvg_amd", "csrc")
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            t = open(os.path.join(d, f)).read()
            t = re.sub(r"/\*.*?\*/", "", t, flags=re.S)
            out[f] = re.sub(r"//[^\n]*", "", t)
    return out


def _definitions(text, name):
    """how often `name(parameters) {` occurs: a function definition, as opposed to a call or a using-declaration"""
    n = 0
    for m in re.finditer(r"(?<![\w.])%s\s*\(" % name, text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        n += re.match(r"\s*\{", text[i:]) is not None
    return n


def test_mfma_operand_layout_is_stated_once():
    """The 32 x 32 MFMA row map and the image <-> operand accessors are a contract between the host-side weight packers and
    every kernel (csrc/mfma_frag.h): one definition of each in csrc, and the row-map formula written out once, so that a fix
    or a layout change cannot leave a private copy behind.  Finds duplication only; scripts/isa_diff.py checks the code."""
    code = _csrc_code()
    where = lambda count: {f: count(t) for f, t in code.items() if count(t)}
    for name in ("rowmap", "row_frag", "col_frag", "pack_regs", "stage_rows", "load_rows", "unpack8", "pack8"):
        assert where(lambda t: _definitions(t, name)) == {"mfma_frag.h": 1}, name
    assert where(lambda t: len(re.findall(r"\bunion\s+Frag8\s*\{", t))) == {"mfma_frag.h": 1}
    # the 8 x bf16 operand vector, under whatever name
    assert where(lambda t: len(re.findall(r"\btypedef\s+__bf16\s+\w+\s+__attribute__\s*\(\(\s*ext_vector_type\(8\)", t))) == {"mfma_frag.h": 1}
    # (r & 3) + 8 * (r >> 2) + 4 * h2, whatever the operands are called: once, in the header.  Kept apart, by name and count:
    # the C-tile row index of the two tiled GEMMs, where the terms are part of a longer sum `m0 + wm * 64 + i * 32 + ...` -
    # hipcc allocates the registers of all 24 kernels differently for any spelling of that sum which calls rowmap()
    kept = {"gemm.hip": 2, "gemm_bf16.hip": 2}
    formula = r"\(\s*(\w+)\s*&\s*3\s*\)\s*\+\s*8\s*\*\s*\(\s*\1\s*>>\s*2\s*\)\s*\+\s*4\s*\*"
    assert where(lambda t: len(re.findall(formula, t))) == {"mfma_frag.h": 1, **kept}


def test_geometry_tier_is_stated_once():
    """The token layout, the flag scan and the curve math are a contract between sample_points, the rasteriser, their
    backwards and the canonical path order (csrc/svg_seq.h): one definition of each in csrc, and one Chamfer sweep and slice
    kernel under a template flag.  Finds duplication only; scripts/isa_diff.py checks the code
    (profiles/geometry_header_isa.log)."""
    code = _csrc_code()
    where = lambda count: {f: count(t) for f, t in code.items() if count(t)}
    hdr = {"svg_seq.h": 1}
    # the scan (under any prefix), its three flags, the count clamp, the start point
    assert where(lambda t: len(re.findall(r"\b\w*flag_scan\s*\([^;{]*\)\s*\{", t))) == hdr
    for name in ("is_drawing", "sequence_draws", "subpath_ends", "chamfer_count", "start_point", "sequence_args_ok"):
        assert where(lambda t: _definitions(t, name)) == hdr, name
    clamp = r"min\s*\(\s*\(long long\)\s*max\s*\(\s*\w+\s*\[\s*\w+\s*\]\s*,\s*0\s*\)\s*,\s*\w+\s*\)"
    assert where(lambda t: len(re.findall(clamp, t))) == hdr
    # the power basis with its Horner evaluation, and the backward accumulator with its row store
    assert where(lambda t: len(re.findall(r"\bstruct\s+CubicPower\s*\{", t))) == hdr
    assert where(lambda t: len(re.findall(r"\bstruct\s+ArgRowGrad\s*\{", t))) == hdr
    horner = r"fmaf\s*\(\s*fmaf\s*\(\s*fmaf\s*\(\s*c3x\s*,"
    assert where(lambda t: len(re.findall(horner, t))) == hdr
    # Kept apart, by name and count: hipcc orders raster_segments_kernel and raster_segments_bwd_kernel differently with
    # start_point's two selects and with the struct (or its updates as functions), so raster.hip keeps its one-branch start
    # point and the accumulator written out (the Bernstein weights and the row store once more)
    bernstein = r"3\.0\s*\*\s*w\s*\*\s*w\s*\*\s*z"
    assert where(lambda t: len(re.findall(bernstein, t))) == {**hdr, "raster.hip": 1}
    assert where(lambda t: len(re.findall(r"\brow\s*\[\s*\w+\s*\]\s*=\s*\(float\)\s*c1x", t))) == {**hdr, "raster.hip": 1}
    assert where(lambda t: len(re.findall(r"\?\s*make_float2\s*\([^;]*-\s*N_ARGS\s*\]", t))) == {"raster.hip": 1}
    # one Chamfer sweep and one slice kernel
    assert where(lambda t: len(re.findall(r"\bvoid\s+chamfer_sweep\w*\s*\(", t))) == {"metrics.hip": 1}
    assert where(lambda t: len(re.findall(r"\bvoid\s+chamfer\w*_slice_kernel\s*\(", t))) == {"metrics.hip": 1}
    # the vocabulary: the argument count and the `l` / `c` ids, under any name
    assert where(lambda t: len(re.findall(r"\bconstexpr\s+int\s+[^;]*\bN_ARGS\s*=", t))) == hdr
    ids = r"\bconstexpr\s+int\s+[^;]*\b\w*L\s*=\s*1\s*,\s*\w*C\s*=\s*2\b"
    assert where(lambda t: len(re.findall(ids, t))) == hdr
