"""The plain GroupNorm of csrc/cgic_norm.hip and csrc/cgic_norm_bwd.hip (ABI 21) without a GPU.

The plans.  cgic_group_norm / _train / _backward are the plans of csrc/cgic_norm_plan.h and cgic_norm_bwd_plan.h with their `plain`
flag set.  tests/host/group_norm_plan_main.cpp is compiled with the host compiler alone -- once plainly, once with
-fsanitize=address,undefined -- and run as a program over the tables below, whose rows were worked out by hand with the rules in
tests/test_norm_plan_host.py and tests/test_norm_bwd_plan_host.py; the plain backward keeps 2 plane sums per (channel, tile) and no
dz partials: workspace = B * C * ceil(H * W / 256) * 2 * 8 + B * C * 2 * 8 bytes.  With the flag set, zq's grid and the five
pointers of zq / conv_y / conv_b (and in the backward their gradients) are not looked at: NULL or nonsense there is accepted; every
other refusal is the modulated call's under the plain call's name.  For equal shapes the form, the unit, the chunks and the forward
workspace are the modulated plan's.

The Python layer.  cg.GroupNorm on the CPU is torch's GroupNorm bit for bit (and x * sigmoid(x) behind it), keeps the state_dict keys
and the parameter objects; the default install() puts none in; the fake kernels give the real ones' dtypes and shapes.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib, norm
import group_norm_ref as gref
import spatial_norm_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -5
F32, F16, BF16 = 0, 1, 2
BIG = 1 << 30

FWD = ("f", "zq", "gn_weight", "gn_bias", "wy", "by", "wb", "bb", "out", "ws", "stats")
BWD = ("f", "go", "zq", "stats", "gn_weight", "gn_bias", "wy", "by", "wb", "bb", "df", "dzq", "dgn_weight", "dgn_bias", "dwy", "dby", "dwb", "dbb", "ws")
GONE_FWD = ("zq", "wy", "by", "wb", "bb")
GONE_BWD = ("zq", "wy", "by", "wb", "bb", "dzq", "dwy", "dby", "dwb", "dbb")
BASE = {k: (i + 1) << 32 for i, k in enumerate(dict.fromkeys(FWD + BWD))}          # 4 GiB apart


def _addresses(order, gone, plain, addr):
    a = {k: (0 if plain and k in gone else BASE[k]) for k in order}
    for key, v in addr.items():
        a[key] = v[1] if isinstance(v, tuple) else BASE[key] + v
    return a


def fwd(name, want, dt_in, dt_out, B, C, H, W, plain=1, hq=0, wq=0, groups=32, ws_bytes=BIG, train=False, **addr):
    """addr: f=+8 style byte offsets from the tensor's base, or absolute addresses as ("abs", value)"""
    a = _addresses(FWD, GONE_FWD, plain, addr)
    if not train and "stats" not in addr:
        a["stats"] = 0
    line = " ".join(str(v) for v in (0, plain, dt_in, dt_out, B, C, H, W, hq, wq, groups, *(a[k] for k in FWD[:10]), ws_bytes, a["stats"]))
    return pytest.param(line, want, id="fwd-" + name)


def bwd(name, want, dt_in, dt_go, dt_df, B, C, H, W, plain=1, hq=0, wq=0, groups=32, ws_bytes=BIG, **addr):
    a = _addresses(BWD, GONE_BWD, plain, addr)
    line = " ".join(str(v) for v in (1, plain, dt_in, dt_go, dt_df, B, C, H, W, hq, wq, groups, *(a[k] for k in BWD), ws_bytes))
    return pytest.param(line, want, id="bwd-" + name)


def err(code, why):
    return dict(err=code, why=why)


F, OUT = BASE["f"], BASE["out"]
PAIR = "group_norm: out_dtype %d with in_dtype %d (CGIC_DT_F32 or the features' own type)"
OVERLAP = "group_norm: out overlaps an input (only out == f with equal types, the in-place form, may)"
WS = "group_norm: workspace of %d bytes, need 2304 (cgic_spatial_norm_workspace_bytes)"
ONE = dict(form=1, unit=4, span=96, spans=128, grid_one=128, lds=384 + 128, workspace=0, ymul=1, ydiv=1, xmul=1, xdiv=1, mg_w=357913942, mg_y=0, mg_x=0, zq_vec=0)
TWO = dict(form=2, unit=4, span=96, spans=96, chunks=1, chunk_units=24, grid_stats=96, grid_apply=96, parts=1, workspace=2304, zq_vec=0)
CASES = [
    # ---- the flag set, zq's grid 0x0 and its five pointers NULL: accepted, both forms, every type pair
    fwd("one-4x32x8x12", ONE, F32, F32, 4, 32, 8, 12),
    fwd("two-3x32x8x12", TWO, F32, F32, 3, 32, 8, 12),
    fwd("two-1x64x136x128", dict(form=2, unit=4, span=34816, spans=32, chunks=32, chunk_units=272, grid_apply=320, parts=5, workspace=32 * 65 * 8),
        F32, F32, 1, 64, 136, 128),
    fwd("one-f16-unit8", dict(form=1, unit=8, span=512, spans=128, lds=1024 + 128), F16, F16, 4, 32, 16, 32),
    fwd("bf16-to-f32-w10-unit2", dict(form=2, unit=2, span=120, spans=32, workspace=32 * 3 * 8), BF16, F32, 1, 64, 6, 10),
    fwd("in-place", dict(form=1, in_place=1), F16, F16, 4, 32, 8, 12, out=("abs", F)),
    fwd("empty-batch", dict(form=0, unit=0, spans=0, workspace=0), F32, F32, 0, 32, 8, 12, ws_bytes=0, f=("abs", 0), gn_weight=("abs", 0),
        gn_bias=("abs", 0), out=("abs", 0), ws=("abs", 0)),
    # ---- ... and nonsense there is not looked at: a zq grid at no ratio, pointers that are misaligned or lie on out
    fwd("zq-fields-ignored", ONE, F32, F32, 4, 32, 8, 12, hq=5, wq=-7, zq=("abs", OUT), wy=("abs", 3), by=("abs", F + 4), wb=("abs", OUT + 8), bb=("abs", 1)),
    fwd("train", TWO, F32, F32, 3, 32, 8, 12, train=True),
    fwd("train-stats-on-a-conv-pointer", TWO, F32, F32, 3, 32, 8, 12, train=True, wy=("abs", BASE["stats"]), zq=("abs", BASE["stats"] + 4)),
    # ---- every other refusal, under the plain call's name
    fwd("types-01", err(UNSUPPORTED, PAIR % (1, 0)), F32, F16, 1, 32, 2, 16),
    fwd("types-12", err(UNSUPPORTED, PAIR % (2, 1)), F16, BF16, 1, 32, 2, 16),
    fwd("types-1-1", err(INVALID, PAIR % (-1, 1)), F16, -1, 1, 32, 2, 16),
    fwd("types-30", err(INVALID, "group_norm: in_dtype 3 (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)"), 3, F32, 1, 32, 2, 16),
    fwd("B-1", err(INVALID, "group_norm: features [-1,32,8,12]"), F32, F32, -1, 32, 8, 12),
    fwd("48-in-32", err(INVALID, "group_norm: 48 channels in 32 groups"), F32, F32, 1, 48, 8, 12),
    fwd("beyond-2^31", err(UNSUPPORTED, "group_norm: a group of 1 x 65536x65536 elements is beyond 2^31"), F32, F32, 1, 32, 65536, 65536),
    fwd("NULL-gn_bias", err(INVALID, "group_norm: NULL tensor"), F32, F32, 1, 32, 8, 12, gn_bias=("abs", 0)),
    fwd("NULL-out", err(INVALID, "group_norm: NULL tensor"), F16, F16, 1, 32, 8, 12, out=("abs", 0)),
    fwd("misaligned-f16+1", err(INVALID, "group_norm: a pointer is not aligned to its 2-byte element"), F16, F32, 1, 32, 2, 16, f=1),
    fwd("misaligned-gn_weight+2", err(INVALID, "group_norm: a pointer is not aligned to its 4-byte element"), F16, F16, 1, 32, 2, 16, gn_weight=2),
    fwd("misaligned-out32+2", err(INVALID, "group_norm: a pointer is not aligned to its 4-byte element"), BF16, F32, 1, 32, 2, 16, out=2),
    fwd("f32-out-on-f16-f", err(INVALID, OVERLAP), F16, F32, 1, 32, 8, 12, out=("abs", F)),
    fwd("out-inside-f", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, out=("abs", F + 16)),
    fwd("out-on-gn_weight", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, out=("abs", BASE["gn_weight"] - 12288 + 4)),
    fwd("ws-exact", TWO, F32, F32, 3, 32, 8, 12, ws_bytes=2304),
    fwd("ws-one-short", err(CAPACITY, WS % 2303), F32, F32, 3, 32, 8, 12, ws_bytes=2303),
    fwd("ws-NULL", err(CAPACITY, WS % 0), F32, F32, 3, 32, 8, 12, ws=("abs", 0)),
    fwd("ws+4", err(INVALID, "group_norm: the workspace is not aligned to 8 bytes"), F32, F32, 3, 32, 8, 12, ws=4),
    fwd("ws-on-out", err(INVALID, "group_norm: the workspace overlaps a tensor of the call"), F32, F32, 3, 32, 8, 12, ws=("abs", OUT + 64)),
    fwd("ws-ends-in-f", err(INVALID, "group_norm: the workspace overlaps a tensor of the call"), F32, F32, 3, 32, 8, 12, ws=("abs", F - 2296)),
    fwd("train-stats+2", err(INVALID, "group_norm_train: stats is not aligned to its 4-byte element"), F32, F32, 3, 32, 8, 12, train=True, stats=2),
    fwd("train-stats-in-out", err(INVALID, "group_norm_train: stats overlaps another tensor of the call"), F32, F32, 3, 32, 8, 12, train=True,
        stats=("abs", OUT + 36860)),
    fwd("train-stats-on-gn_bias", err(INVALID, "group_norm_train: stats overlaps another tensor of the call"), F32, F32, 3, 32, 8, 12, train=True,
        stats=("abs", BASE["gn_bias"] + 124)),
]

# ---- the backward: [4,64,6,10] fp32 -- a plane of 60 pixels, unit 2, 8 channels per reduce workgroup, one tile;
# workspace = 4 * 64 * 1 * 2 * 8 (sums) + 4 * 64 * 2 * 8 (span) = 8192, no dz
BPLAN = dict(unit=2, span=120, spans=128, chan_block=8, chan_blocks=8, threads_reduce=64, tiles=1, tiles_max=1, grid_reduce=32, grid_sums=1, grid_dzq=0,
             grid_apply=256, parts=1, need_dz=0, need_conv=0, need_df=1, in_place=0, sums=2, off_sums=0, off_span=4096, off_dz=8192, workspace=8192, zq_vec=0)
BNAME = "group_norm_backward: "
BWS = BNAME + "workspace of %d bytes, need 8192 (cgic_group_norm_backward_workspace_bytes)"
BOVER = BNAME + "an output overlaps another tensor of the call (only df == go with equal types may)"
NO_OUT = dict(df=("abs", 0), dgn_weight=("abs", 0), dgn_bias=("abs", 0))
BCASES = [
    bwd("plain-4x64x6x10", BPLAN, F32, F32, F32, 4, 64, 6, 10),
    bwd("zq-fields-ignored", BPLAN, F32, F32, F32, 4, 64, 6, 10, hq=5, wq=-7, zq=("abs", 3), wy=("abs", BASE["df"]), dzq=("abs", BASE["df"] + 8),
        dwy=("abs", BASE["f"]), dby=("abs", 1), dwb=("abs", BASE["go"]), dbb=("abs", BASE["ws"])),
    bwd("ws-exact", BPLAN, F32, F32, F32, 4, 64, 6, 10, ws_bytes=8192),
    bwd("only-dgn_bias", {**BPLAN, "need_df": 0, "grid_apply": 0, "parts": 0}, F32, F32, F32, 4, 64, 6, 10, df=("abs", 0), dgn_weight=("abs", 0)),
    bwd("only-df", BPLAN, F32, F32, F32, 4, 64, 6, 10, dgn_weight=("abs", 0), dgn_bias=("abs", 0)),
    bwd("in-place-f16", {**BPLAN, "in_place": 1}, F16, F16, F16, 4, 64, 6, 10, df=("abs", BASE["go"])),
    bwd("big-1x64x136x128-f16", dict(unit=8, chan_block=16, chan_blocks=4, threads_reduce=256, tiles=9, tiles_max=68, sums=2, off_span=64 * 68 * 16,
                                     off_dz=64 * 68 * 16 + 64 * 16, workspace=64 * 68 * 16 + 64 * 16, grid_dzq=0), F16, F32, F16, 1, 64, 136, 128),
    bwd("types-go", err(UNSUPPORTED, BNAME + "go_dtype 1 with in_dtype 0 (CGIC_DT_F32 or the features' own type)"), F32, F16, F32, 4, 64, 6, 10),
    bwd("types-df", err(UNSUPPORTED, BNAME + "df_dtype 2 with in_dtype 1 (CGIC_DT_F32 or the features' own type)"), F16, F16, BF16, 4, 64, 6, 10),
    bwd("types-in", err(INVALID, "group_norm: in_dtype 7 (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)"), 7, F32, F32, 4, 64, 6, 10),
    bwd("48-in-32", err(INVALID, "group_norm: 48 channels in 32 groups"), F32, F32, F32, 4, 48, 6, 10),
    bwd("empty-batch", err(INVALID, BNAME + "an empty batch"), F32, F32, F32, 0, 64, 6, 10),
    bwd("NULL-stats", err(INVALID, BNAME + "NULL input"), F32, F32, F32, 4, 64, 6, 10, stats=("abs", 0)),
    bwd("NULL-go", err(INVALID, BNAME + "NULL input"), F32, F32, F32, 4, 64, 6, 10, go=("abs", 0)),
    bwd("nothing-wanted", err(INVALID, BNAME + "no gradient is wanted (every output is NULL)"), F32, F32, F32, 4, 64, 6, 10, **NO_OUT),
    bwd("nothing-wanted-conv-gradients-do-not-count", err(INVALID, BNAME + "no gradient is wanted (every output is NULL)"), F32, F32, F32, 4, 64, 6, 10,
        **NO_OUT, dwy=("abs", BASE["dwy"]), dzq=("abs", BASE["dzq"])),
    bwd("misaligned-go16+1", err(INVALID, BNAME + "a pointer is not aligned to its 2-byte element"), F16, F16, F16, 4, 64, 6, 10, go=1),
    bwd("misaligned-dgn_bias+2", err(INVALID, BNAME + "a pointer is not aligned to its 4-byte element"), F32, F32, F32, 4, 64, 6, 10, dgn_bias=2),
    bwd("df-on-f", err(INVALID, BOVER), F32, F32, F32, 4, 64, 6, 10, df=("abs", F)),
    bwd("f32-df-on-f16-go", err(INVALID, BOVER), F16, F16, F32, 4, 64, 6, 10, df=("abs", BASE["go"])),
    bwd("dgn_weight-on-stats", err(INVALID, BOVER), F32, F32, F32, 4, 64, 6, 10, dgn_weight=("abs", BASE["stats"] + 1020)),
    bwd("dgn_bias-on-dgn_weight", err(INVALID, BOVER), F32, F32, F32, 4, 64, 6, 10, dgn_bias=("abs", BASE["dgn_weight"] + 252)),
    bwd("ws-one-short", err(CAPACITY, BWS % 8191), F32, F32, F32, 4, 64, 6, 10, ws_bytes=8191),
    bwd("ws-NULL", err(CAPACITY, BWS % 0), F32, F32, F32, 4, 64, 6, 10, ws=("abs", 0)),
    bwd("ws+8", err(INVALID, BNAME + "the workspace is not aligned to 16 bytes"), F32, F32, F32, 4, 64, 6, 10, ws=8),
    bwd("ws-on-df", err(INVALID, BNAME + "the workspace overlaps a tensor of the call"), F32, F32, F32, 4, 64, 6, 10, ws=("abs", BASE["df"] + 64)),
    bwd("ws-ends-in-stats", err(INVALID, BNAME + "the workspace overlaps a tensor of the call"), F32, F32, F32, 4, 64, 6, 10, ws=("abs", BASE["stats"] - 8176)),
]
ALL = CASES + BCASES


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "group_norm_plan_main.cpp"), "-o", exe])
    return exe


def _parse(line):
    if line.startswith("err="):
        code, why = line.split(" why=", 1)
        return dict(err=int(code[4:]), why=why)
    return {k: int(v) for k, v in (t.split("=", 1) for t in line.split())}


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return [_parse(g) for g in got]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("group_norm_plan"), [], "group_norm_plan_main")


@pytest.fixture(scope="module")
def plans(exe):
    return dict(zip((c.id for c in ALL), _run(exe, [c.values[0] for c in ALL])))


def test_abi_21():
    assert _lib.lib().cgic_abi_version() >= 21


def test_the_tables_have_no_two_rows_of_one_name():
    for table in (CASES, BCASES):
        ids = [c.id for c in table]
        assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", ALL)
def test_group_norm_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_group_norm_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    san = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "group_norm_plan_main_san")
    assert dict(zip((c.id for c in ALL), _run(san, [c.values[0] for c in ALL]))) == plans


SHAPES = [(F32, 4, 32, 8, 12), (F32, 3, 32, 8, 12), (F16, 1, 128, 256, 256), (F32, 8, 128, 256, 256), (F16, 8, 512, 16, 16), (F32, 1, 512, 16, 16),
          (F32, 1, 64, 136, 128), (BF16, 4, 32, 34, 68), (F32, 1, 32, 3, 5), (F16, 64, 544, 32, 32)]


def test_the_form_the_chunks_and_the_workspace_are_the_modulated_plans(exe):
    """the same shapes planned with and without the flag (the modulated call at ratio 1 on a real zq): everything the shape decides,
    and the unit and the grids, are equal; the backward differs in its sums and its workspace only"""
    lines = []
    for dt, B, C, H, W in SHAPES:
        for plain in (1, 0):
            lines.append(fwd("x", None, dt, dt, B, C, H, W, plain=plain, hq=H, wq=W).values[0])
            lines.append(bwd("x", None, dt, dt, dt, B, C, H, W, plain=plain, hq=H, wq=W).values[0])
    got = _run(exe, lines)
    for i, shape in enumerate(SHAPES):
        pf, pb, mf, mb = got[4 * i:4 * i + 4]
        assert all("err" not in g for g in (pf, pb, mf, mb)), shape
        same = ("form", "unit", "span", "spans", "chunks", "chunk_units", "grid_one", "grid_stats", "grid_apply", "parts", "lds", "workspace", "mg_w")
        assert {k: pf[k] for k in same} == {k: mf[k] for k in same}, shape
        assert pf["zq_vec"] == 0 and mf["zq_vec"] == 1
        same = ("unit", "span", "spans", "chan_block", "chan_blocks", "threads_reduce", "tiles", "tiles_max", "grid_reduce", "grid_apply", "parts", "need_df")
        assert {k: pb[k] for k in same} == {k: mb[k] for k in same}, shape
        assert (pb["sums"], mb["sums"], pb["grid_dzq"], pb["need_dz"], pb["need_conv"]) == (2, 12, 0, 0, 0) and mb["need_dz"] == mb["need_conv"] == 1
        B, C, H, W = shape[1:]
        assert pb["workspace"] == B * C * pb["tiles_max"] * 16 + B * C * 16 and pb["workspace"] < mb["workspace"]
        lib = _lib.lib()
        assert lib.cgic_group_norm_backward_workspace_bytes(shape[0], B, C, H, W, 32) == pb["workspace"]
        assert lib.cgic_spatial_norm_backward_workspace_bytes(shape[0], B, C, H, W, 32) == mb["workspace"]
        assert lib.cgic_spatial_norm_workspace_bytes(shape[0], B, C, H, W, 32) == pf["workspace"]
        assert lib.cgic_spatial_norm_one_launch(shape[0], B, C, H, W, 32) == (pf["form"] == 1)


def test_the_library_refuses_as_the_plan_does_before_any_launch():
    """a refused call enqueues nothing: it can be made without a device, with made-up addresses (never dereferenced)"""
    def refused(entry, code, text, *args):
        with pytest.raises(cg.CgicError) as got:
            _lib.call(entry, *args)
        assert got.value.code == code and text in str(got.value), str(got.value)

    f, gw, gb, out, ws, st, go, df = (BASE[k] for k in ("f", "gn_weight", "gn_bias", "out", "ws", "stats", "go", "df"))
    refused("cgic_group_norm", UNSUPPORTED, PAIR % (1, 0), f, F32, 1, 32, 8, 12, 32, 1e-6, gw, gb, 0, out, F16, ws, BIG, None)
    refused("cgic_group_norm", INVALID, OVERLAP, f, F16, 1, 32, 8, 12, 32, 1e-6, gw, gb, 1, f, F32, ws, BIG, None)
    refused("cgic_group_norm", CAPACITY, WS % 0, f, F32, 3, 32, 8, 12, 32, 1e-6, gw, gb, 0, out, F32, None, 0, None)
    refused("cgic_group_norm", INVALID, "group_norm: NULL tensor", f, F32, 1, 32, 8, 12, 32, 1e-6, None, gb, 0, out, F32, ws, BIG, None)
    refused("cgic_group_norm", INVALID, "group_norm: eps -1", f, F32, 1, 32, 8, 12, 32, -1.0, gw, gb, 0, out, F32, ws, BIG, None)
    refused("cgic_group_norm", INVALID, "group_norm: 48 channels in 32 groups", f, F32, 1, 48, 8, 12, 32, 1e-6, gw, gb, 0, out, F32, ws, BIG, None)
    refused("cgic_group_norm_train", INVALID, "group_norm_train: stats is NULL", f, F32, 3, 32, 8, 12, 32, 1e-6, gw, gb, 0, out, F32, None, ws, BIG, None)
    refused("cgic_group_norm_backward", CAPACITY, BWS % 100, f, F32, go, F32, 4, 64, 6, 10, 32, st, gw, gb, 1, df, F32, None, None, ws, 100, None)
    refused("cgic_group_norm_backward", INVALID, BNAME + "no gradient is wanted", f, F32, go, F32, 4, 64, 6, 10, 32, st, gw, gb, 1, None, F32, None, None, ws, BIG, None)
    assert _lib.call("cgic_group_norm", None, F32, 0, 32, 8, 12, 32, 1e-6, None, None, 0, None, F32, None, 0, None) == OK


# ---------------------------------------------------------------------------- the reference, the module, install(), the ops
def test_the_restatement_is_torchs_float64_group_norm():
    rng = np.random.default_rng(3)
    for C, H, W in ((32, 3, 5), (64, 6, 10), (128, 4, 4)):
        x = gref.make_inputs(rng, 2, C, H, W)
        for swish in (False, True):
            want = torch.nn.functional.group_norm(x["f"].double(), 32, x["gn_w"].double(), x["gn_b"].double(), 1e-6)
            want = want * torch.sigmoid(want) if swish else want
            got = gref.restatement(x["f"], x["gn_w"], x["gn_b"], swish=swish)
            assert float((got - want).abs().max()) < 1e-12
            assert 0 < gref.e_ref(got, x["f"], x["gn_w"], x["gn_b"], swish=swish) < 1e-5


def _pair(C=64, seed=5):
    theirs = sref.randomize(torch.nn.GroupNorm(num_groups=32, num_channels=C, eps=1e-6, affine=True), seed)
    return theirs, norm.GroupNorm.adopt(theirs)


def test_the_module_on_the_cpu_is_torchs_bit_for_bit():
    theirs, mine = _pair()
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 64, 6, 10)).astype(np.float32))
    assert mine._route(x) == "torch" and not mine.uses_kernel(x) and not mine.uses_backward_kernel(x)
    want = theirs(x)
    assert torch.equal(mine(x), want)
    assert torch.equal(mine(x, swish=True), want * torch.sigmoid(want))
    assert mine(x, out_dtype=torch.bfloat16).dtype == torch.bfloat16
    built = norm.GroupNorm(32, 64, eps=1e-6)
    built.load_state_dict(theirs.state_dict())
    assert torch.equal(built(x), want) and built.eps == 1e-6 and built.num_groups == 32
    g1, = torch.autograd.grad(mine(x.requires_grad_()).square().sum(), x)
    g2, = torch.autograd.grad(theirs(x).square().sum(), x)
    assert torch.equal(g1, g2)


def test_adopt_keeps_the_keys_the_parameter_objects_and_the_mode():
    theirs, mine = _pair()
    assert isinstance(mine, torch.nn.GroupNorm) and type(mine) is norm.GroupNorm
    assert list(mine.state_dict()) == list(theirs.state_dict()) == ["weight", "bias"]
    assert mine.weight is theirs.weight and mine.bias is theirs.bias and mine.training == theirs.training
    assert (mine.num_groups, mine.num_channels, mine.eps, mine.affine) == (32, 64, 1e-6, True) and not mine.backward_kernel
    assert norm.GroupNorm.adopt(theirs.eval()).training is False
    plain = norm.GroupNorm.adopt(torch.nn.GroupNorm(4, 8, affine=False))
    assert plain.weight is None and plain._route(torch.zeros(1, 8, 2, 2)) == "torch"
    with pytest.raises(TypeError, match="is not a torch.nn.GroupNorm"):
        norm.GroupNorm.adopt(torch.nn.BatchNorm2d(8))


class _Model(torch.nn.Module):
    """what install() touches, as small as it gets: an encoder with plain GroupNorms, a decoder with a SpatialNorm-shaped module"""

    def __init__(self):
        super().__init__()
        self.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
        self.encoder = torch.nn.Module()
        self.encoder.norm_out = torch.nn.GroupNorm(32, 64, eps=1e-6)
        self.encoder.no_affine = torch.nn.GroupNorm(32, 64, affine=False)
        self.decoder = torch.nn.Module()
        self.decoder.norm_out = sref.StandIn(32)


def _kinds(m):
    return [type(c) for c in m.modules()]


def test_install_swaps_group_norms_only_when_asked_and_never_a_spatial_norms_own():
    m = _Model()
    before = [(k, type(c)) for k, c in m.named_modules() if k.startswith(("encoder", "decoder"))]
    cg.install(m)
    assert [(k, type(c)) for k, c in m.named_modules() if k.startswith(("encoder", "decoder"))] == before       # today's module tree
    assert not any(isinstance(c, (norm.GroupNorm, cg.ResnetBlock)) for c in m.modules())
    params = {k: p for k, p in m.named_parameters() if not k.startswith("quantize")}         # (install() builds a new quantiser)
    cg.install(m, patch_group_norms=True)
    assert type(m.encoder.norm_out) is norm.GroupNorm and not m.encoder.norm_out.backward_kernel
    assert type(m.encoder.no_affine) is torch.nn.GroupNorm
    assert type(m.decoder.norm_out) is sref.StandIn and type(m.decoder.norm_out.norm_layer) is torch.nn.GroupNorm
    after = {k: p for k, p in m.named_parameters() if not k.startswith("quantize")}
    assert list(after) == list(params) and all(p is params[k] for k, p in after.items())
    m = _Model()
    cg.install(m, patch_norms=True, patch_group_norms=True, norm_backward=True)
    assert type(m.decoder.norm_out) is norm.SpatialNorm and type(m.decoder.norm_out.norm_layer) is torch.nn.GroupNorm
    assert m.encoder.norm_out.backward_kernel and m.decoder.norm_out.backward_kernel
    assert norm.patch_group_norms(m) == 0                                                                       # again: nothing left to swap


@pytest.mark.parametrize("dtype, half_out", [(torch.float32, False), (torch.float16, False), (torch.float16, True), (torch.bfloat16, True)])
def test_the_fake_kernels_give_the_dtypes_and_shapes(dtype, half_out):
    with FakeTensorMode():
        f = torch.empty(2, 64, 6, 10, device="cuda", dtype=dtype)
        w = torch.empty(64, device="cuda")
        out = torch.ops.cgic.group_norm(f, w, w, 32, 1e-6, True, half_out)
        tout, stats = torch.ops.cgic.group_norm_train(f, w, w, 32, 1e-6, False, half_out)
    want = dtype if half_out else torch.float32
    assert out.shape == tout.shape == f.shape and out.dtype == tout.dtype == want and out.device.type == "cuda"
    assert stats.shape == (2 * 32, 2) and stats.dtype == torch.float32


def test_the_raw_calls_check_before_they_touch_a_pointer():
    f, w = torch.zeros(1, 48, 2, 2), torch.zeros(48)
    assert norm.GN_GRADS == ("f", "gn_weight", "gn_bias")
    with pytest.raises(ValueError, match="group_norm: 48 channels in 32 groups"):
        norm._check_call("group_norm", f, None, (w, w), 32)
    with pytest.raises(ValueError, match="group_norm: gn_bias .* expected 64 floating-point values"):
        norm._check_call("group_norm", torch.zeros(1, 64, 2, 2), None, (torch.zeros(64), w), 32)
    with pytest.raises(TypeError, match="group_norm: features torch.int32"):
        norm._check_call("group_norm", torch.zeros(1, 64, 2, 2, dtype=torch.int32), None, (w, w), 32)
