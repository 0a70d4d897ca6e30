"""The launch plan of cgic_spatial_norm (csrc/cgic_norm_plan.h) without a GPU: every check of the call, the form, the unit, the
chunking and the grids.  The header is plain C++17: tests/host/norm_plan_main.cpp is compiled with the host compiler alone -- once
plainly, once with -fsanitize=address,undefined -- and run as a program over the table below, whose rows were worked out by hand:
  span = (C / groups) * H * W elements, spans = B * groups;
  one launch (form 1) iff span * sizeof(element) <= 65536 and spans >= 128: grid = spans, LDS = the span rounded up to 16 bytes + 128;
  otherwise two (form 2): chunks = min(span // 1024, ceil(4096 / spans), 32), at least 1; workspace = spans * (2 * chunks + 1) * 8;
      chunk_units = ceil(span / unit / chunks); the statistics' grid = spans * chunks;
      parts = ceil(H * W / unit / 1024); the apply's grid = min(B * C * parts, 16384);
  unit = the largest of 8 (halves only), 4, 2 that divides W and whose access (unit elements, 16 bytes at most) both f and out are
      aligned to; else 1;
  the nearest index of an axis: div = n / nq when n % nq == 0 (up), else mul = nq / n when nq % n == 0 (down), else refused;
  the kernels' divisions by W, ydiv and xdiv are multiplications by ceil(2^32 / d) where (largest dividend) * d < 2^32 and d > 1
      (mg_w, mg_y, mg_x; 0: the kernel divides); zq_vec: x at ratio 1 and zq 16-byte aligned."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -5
F32, F16, BF16 = 0, 1, 2
ORDER = ("f", "zq", "gn_weight", "gn_bias", "wy", "by", "wb", "bb", "out", "ws")
BASE = {k: (i + 1) << 32 for i, k in enumerate(ORDER)}          # 4 GiB apart
OVERLAP = "spatial_norm: out overlaps an input (only out == f with equal types, the in-place form, may)"
BIG = 1 << 30


def case(name, want, dt_in, dt_out, B, C, H, W, hq, wq, groups=32, ws_bytes=BIG, **addr):
    """addr: f=+8 style byte offsets from the tensor's base, or absolute addresses as ("abs", value)"""
    a = dict(BASE)
    for key, v in addr.items():
        a[key] = v[1] if isinstance(v, tuple) else BASE[key] + v
    line = " ".join(str(v) for v in (dt_in, dt_out, B, C, H, W, hq, wq, groups, *(a[key] for key in ORDER), ws_bytes))
    return pytest.param(line, want, id=name)


def one(unit, span, spans, lds, **kw):
    return dict(form=1, unit=unit, span=span, spans=spans, grid_one=spans, lds=lds, workspace=0, threads_one=512, **kw)


def two(unit, span, spans, chunks, chunk_units, grid_apply, parts=1, **kw):
    return dict(form=2, unit=unit, span=span, spans=spans, chunks=chunks, chunk_units=chunk_units, grid_stats=spans * chunks,
                grid_apply=grid_apply, parts=parts, workspace=spans * (2 * chunks + 1) * 8, threads=256, **kw)


def err(code, why):
    return dict(err=code, why=why)


F = BASE["f"]
NULLS = {k: ("abs", 0) for k in ORDER}
CASES = [
    # ---- the form, either side of each condition
    case("one-4x32x8x12", one(4, 96, 128, 384 + 128, ymul=1, ydiv=4, xmul=1, xdiv=4), F32, F32, 4, 32, 8, 12, 2, 3),
    case("two-3x32x8x12-too-few-spans", two(4, 96, 96, 1, 24, 96), F32, F32, 3, 32, 8, 12, 2, 3),
    case("one-64x512x32x32-f16", one(8, 16384, 2048, 32768 + 128), F16, F16, 64, 512, 32, 32, 64, 64),
    case("one-64x512x32x32-f32-at-the-budget", one(4, 16384, 2048, 65536 + 128, ymul=2, xmul=2, ydiv=1, xdiv=1), F32, F32, 64, 512, 32, 32, 64, 64),
    case("two-64x544x32x32-f32-past-the-budget", two(4, 17408, 2048, 2, 2176, 16384), F32, F32, 64, 544, 32, 32, 64, 64),
    case("two-64x512x64x64-f32", two(4, 65536, 2048, 2, 8192, 16384), F32, F32, 64, 512, 64, 64, 64, 64),
    case("two-1x512x16x16-down4", two(4, 4096, 32, 4, 256, 512, ymul=4, ydiv=1, xmul=4, xdiv=1), F32, F32, 1, 512, 16, 16, 64, 64),
    case("two-1x128x256x256-f16", two(8, 262144, 32, 32, 1024, 1024, parts=8, ydiv=4, xdiv=4), F16, F32, 1, 128, 256, 256, 64, 64),
    case("two-1x64x136x128", two(4, 34816, 32, 32, 272, 320, parts=5), F32, F32, 1, 64, 136, 128, 34, 32),
    case("two-4x64x136x128-enough-spans-but-too-long", two(4, 34816, 128, 32, 272, 1280, parts=5), F32, F32, 4, 64, 136, 128, 34, 32),
    case("two-1x32x34x68", two(4, 2312, 32, 2, 289, 32, ydiv=2, xdiv=4), F32, F32, 1, 32, 34, 68, 17, 17),
    case("two-1x32x33x68-short-last-chunk", two(4, 2244, 32, 2, 281, 32), F32, F32, 1, 32, 33, 68, 33, 68),
    case("one-needs-no-workspace", one(4, 96, 128, 512), F32, F32, 4, 32, 8, 12, 2, 3, ws=("abs", 0), ws_bytes=0),
    # ---- the axes independently: y sub-sampled 4x, x up-sampled 2x
    case("down4-up2", two(4, 32, 32, 1, 8, 64, ymul=4, ydiv=1, xmul=1, xdiv=2), F32, F32, 1, 64, 2, 8, 8, 4),
]
# ---- the magic multipliers and the vector reads of zq: 2^32 = 4294967296; / 12 = 357913941.3, / 4 = 1073741824, / 3 = 1431655765.3
CASES += [
    case("magic-8x12-up4", one(4, 96, 128, 512, mg_w=357913942, mg_y=1073741824, mg_x=1073741824, zq_vec=0), F32, F32, 4, 32, 8, 12, 2, 3),
    case("magic-12x12-up3-x1", two(4, 144, 32, 1, 36, 32, mg_w=357913942, mg_y=1431655766, mg_x=0, zq_vec=1), F32, F32, 1, 32, 12, 12, 4, 12),
    case("magic-x1-zq+4", two(4, 144, 32, 1, 36, 32, mg_x=0, zq_vec=0), F32, F32, 1, 32, 12, 12, 4, 12, zq=4),
    case("magic-down4", two(4, 4096, 32, 4, 256, 512, mg_w=268435456, mg_y=0, mg_x=0, zq_vec=0), F32, F32, 1, 512, 16, 16, 64, 64),
    case("magic-none-past-2^32", two(4, 65536 * 4, 32, 32, 2048, 2048, parts=64, mg_w=0, mg_y=0, mg_x=0, zq_vec=1), F32, F32, 1, 32, 4, 65536, 4, 65536),
]
# ---- the unit by row width (aligned pointers), [1,32,2,W] on zq [1,4,2,W]
for dt, w, unit in ((F32, 2, 2), (F32, 3, 1), (F32, 4, 4), (F32, 6, 2), (F32, 8, 4), (F16, 8, 8), (F16, 12, 4), (F16, 10, 2), (BF16, 5, 1), (BF16, 16, 8)):
    CASES.append(case(f"unit-dt{dt}-w{w}", two(unit, 2 * w, 32, 1, 2 * w // unit, 32), dt, dt, 1, 32, 2, w, 2, w))
# ---- the unit by pointer alignment: halves on [1,32,2,16] (32 elements per span)
for name, unit, dt_out, addr in (("f+2", 1, F32, dict(f=2)), ("f+4", 2, F32, dict(f=4)), ("f+8", 4, F32, dict(f=8)), ("f+16", 8, F32, dict(f=16)),
                                 ("out32+4", 1, F32, dict(out=4)), ("out32+8", 2, F32, dict(out=8)), ("out32+16", 8, F32, dict(out=16)),
                                 ("out16+2", 1, F16, dict(out=2)), ("out16+8", 4, F16, dict(out=8)),
                                 ("zq+4-does-not-matter", 8, F32, dict(zq=4)), ("wy+4-does-not-matter", 8, F32, dict(wy=4))):
    CASES.append(case(f"align-{name}", two(unit, 32, 32, 1, 32 // unit, 32), F16, dt_out, 1, 32, 2, 16, 2, 16, **addr))
CASES += [
    case("align-f32-f+8", two(2, 32, 32, 1, 16, 32), F32, F32, 1, 32, 2, 16, 2, 16, f=8),
    case("align-f32-out+4", two(1, 32, 32, 1, 32, 32), F32, F32, 1, 32, 2, 16, 2, 16, out=4),
    case("misaligned-f16+1", err(INVALID, "spatial_norm: a pointer is not aligned to its 2-byte element"), F16, F32, 1, 32, 2, 16, 2, 16, f=1),
    case("misaligned-f32+2", err(INVALID, "spatial_norm: a pointer is not aligned to its 4-byte element"), F32, F32, 1, 32, 2, 16, 2, 16, f=2),
    case("misaligned-zq+2", err(INVALID, "spatial_norm: a pointer is not aligned to its 4-byte element"), F16, F32, 1, 32, 2, 16, 2, 16, zq=2),
    case("misaligned-out32+2", err(INVALID, "spatial_norm: a pointer is not aligned to its 4-byte element"), BF16, F32, 1, 32, 2, 16, 2, 16, out=2),
    case("misaligned-bb+1", err(INVALID, "spatial_norm: a pointer is not aligned to its 4-byte element"), F16, F16, 1, 32, 2, 16, 2, 16, bb=1),
]
# ---- the type pairs
for dt_in, dt_out in ((F32, F32), (F16, F32), (F16, F16), (BF16, F32), (BF16, BF16)):
    CASES.append(case(f"types-{dt_in}{dt_out}", two(4 if dt_in == F32 else 8, 32, 32, 1, 8 if dt_in == F32 else 4, 32), dt_in, dt_out, 1, 32, 2, 16, 2, 16))
PAIR = "spatial_norm: out_dtype %d with in_dtype %d (CGIC_DT_F32 or the features' own type)"
CASES += [
    case("types-01", err(UNSUPPORTED, PAIR % (1, 0)), F32, F16, 1, 32, 2, 16, 2, 16),
    case("types-02", err(UNSUPPORTED, PAIR % (2, 0)), F32, BF16, 1, 32, 2, 16, 2, 16),
    case("types-12", err(UNSUPPORTED, PAIR % (2, 1)), F16, BF16, 1, 32, 2, 16, 2, 16),
    case("types-21", err(UNSUPPORTED, PAIR % (1, 2)), BF16, F16, 1, 32, 2, 16, 2, 16),
    case("types-1-1", err(INVALID, PAIR % (-1, 1)), F16, -1, 1, 32, 2, 16, 2, 16),
    case("types-30", err(INVALID, "spatial_norm: in_dtype 3 (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)"), 3, F32, 1, 32, 2, 16, 2, 16),
]
# ---- the shapes, in the order of the checks
CASES += [
    case("B-1", err(INVALID, "spatial_norm: features [-1,32,8,12]"), F32, F32, -1, 32, 8, 12, 2, 3),
    case("W0", err(INVALID, "spatial_norm: features [1,32,8,0]"), F32, F32, 1, 32, 8, 0, 2, 3),
    case("48-in-32", err(INVALID, "spatial_norm: 48 channels in 32 groups"), F32, F32, 1, 48, 8, 12, 2, 3),
    case("groups0", err(INVALID, "spatial_norm: 32 channels in 0 groups"), F32, F32, 1, 32, 8, 12, 2, 3, groups=0),
    case("beyond-2^31", err(UNSUPPORTED, "spatial_norm: a group of 1 x 65536x65536 elements is beyond 2^31"), F32, F32, 1, 32, 65536, 65536, 1, 1),
    case("zq-0x3", err(INVALID, "spatial_norm: zq grid 0x3"), F32, F32, 1, 32, 8, 12, 0, 3),
    case("ratio-6-over-4", err(UNSUPPORTED, "spatial_norm: zq 4x3 under features 6x6 (each axis an integer ratio, up or down)"), F32, F32, 1, 32, 6, 6, 4, 3),
    case("ratio-x-4-over-6", err(UNSUPPORTED, "spatial_norm: zq 2x6 under features 4x4 (each axis an integer ratio, up or down)"), F32, F32, 1, 32, 4, 4, 2, 6),
    case("types-before-zq", err(UNSUPPORTED, PAIR % (1, 0)), F32, F16, 1, 32, 6, 6, 4, 3),
    case("groups-16", two(4, 192, 16, 1, 48, 32), F32, F32, 1, 32, 8, 12, 2, 3, groups=16),
    case("empty-batch-NULL", dict(form=0, unit=0, spans=0, workspace=0), F32, F32, 0, 32, 8, 12, 2, 3, ws_bytes=0, **NULLS),
    case("empty-batch-still-checks-the-ratio", err(UNSUPPORTED, "spatial_norm: zq 4x3 under features 6x6 (each axis an integer ratio, up or down)"),
         F32, F32, 0, 32, 6, 6, 4, 3, **NULLS),
    case("NULL-all", err(INVALID, "spatial_norm: NULL tensor"), F32, F32, 1, 32, 8, 12, 2, 3, **NULLS),
    case("NULL-gn_bias", err(INVALID, "spatial_norm: NULL tensor"), F32, F32, 1, 32, 8, 12, 2, 3, gn_bias=("abs", 0)),
    case("NULL-out", err(INVALID, "spatial_norm: NULL tensor"), F16, F16, 1, 32, 8, 12, 2, 3, out=("abs", 0)),
]
# ---- aliasing: [1,32,8,12] = 3072 elements
CASES += [
    case("in-place-f32", two(4, 96, 32, 1, 24, 32, in_place=1), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", F)),
    case("in-place-f16", two(4, 96, 32, 1, 24, 32, in_place=1), F16, F16, 1, 32, 8, 12, 2, 3, out=("abs", F)),
    case("in-place-one-launch", one(4, 96, 128, 192 + 128, in_place=1), BF16, BF16, 4, 32, 8, 12, 2, 3, out=("abs", F)),
    case("f32-out-on-f16-f", err(INVALID, OVERLAP), F16, F32, 1, 32, 8, 12, 2, 3, out=("abs", F)),
    case("out-inside-f", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", F + 16)),
    case("out-ends-inside-f", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", F - 12288 + 16)),
    case("out-before-f", two(4, 96, 32, 1, 24, 32, in_place=0), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", F - 12288)),
    case("out-behind-f", two(4, 96, 32, 1, 24, 32, in_place=0), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", F + 12288)),
    case("out-on-zq", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", BASE["zq"])),
    case("out-on-wb", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", BASE["wb"])),
    case("out-ends-in-bb", err(INVALID, OVERLAP), F32, F32, 1, 32, 8, 12, 2, 3, out=("abs", BASE["bb"] - 12288 + 4)),
]
# ---- the workspace of the two-launch form: [3,32,8,12] needs 96 * 3 * 8 = 2304 bytes
WS = "spatial_norm: workspace of %d bytes, need 2304 (cgic_spatial_norm_workspace_bytes)"
CASES += [
    case("ws-exact", two(4, 96, 96, 1, 24, 96), F32, F32, 3, 32, 8, 12, 2, 3, ws_bytes=2304),
    case("ws-one-short", err(CAPACITY, WS % 2303), F32, F32, 3, 32, 8, 12, 2, 3, ws_bytes=2303),
    case("ws-NULL", err(CAPACITY, WS % 0), F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", 0)),
    case("ws+4", err(INVALID, "spatial_norm: the workspace is not aligned to 8 bytes"), F32, F32, 3, 32, 8, 12, 2, 3, ws=4),
    case("ws-on-out", err(INVALID, "spatial_norm: the workspace overlaps a tensor of the call"), F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", BASE["out"] + 64)),
    case("ws-ends-in-f", err(INVALID, "spatial_norm: the workspace overlaps a tensor of the call"), F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", F - 2296)),
    case("ws-before-f", two(4, 96, 96, 1, 24, 96), F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", F - 2304)),
]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "norm_plan_main.cpp"), "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], input="\n".join(c.values[0] for c in CASES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    parsed = {}
    for c, line in zip(CASES, lines):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            parsed[c.id] = {k: int(v) for k, v in (t.split("=", 1) for t in line.split())}
    return parsed


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("norm_plan"), [], "norm_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_norm_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_norm_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "norm_plan_main_san")
    assert _run(exe) == plans


def test_the_library_answers_as_the_plan_does():
    """cgic_spatial_norm_one_launch / _workspace_bytes are the plan's shape part, and a refused call enqueues nothing: it can be made
    without a device, with made-up addresses (never dereferenced)"""
    import control_gic_amd as cg
    from control_gic_amd import _lib
    lib = _lib.lib()
    assert lib.cgic_spatial_norm_one_launch(F32, 4, 32, 8, 12, 32) == 1 and lib.cgic_spatial_norm_one_launch(F32, 3, 32, 8, 12, 32) == 0
    assert lib.cgic_spatial_norm_one_launch(F32, 64, 512, 32, 32, 32) == 1 and lib.cgic_spatial_norm_one_launch(F32, 64, 544, 32, 32, 32) == 0
    assert lib.cgic_spatial_norm_one_launch(F16, 64, 544, 32, 32, 32) == 1
    assert lib.cgic_spatial_norm_one_launch(F32, 1, 48, 8, 12, 32) == INVALID
    assert "48 channels in 32 groups" in lib.cgic_last_error().decode()
    assert lib.cgic_spatial_norm_workspace_bytes(F32, 3, 32, 8, 12, 32) == 2304 and lib.cgic_spatial_norm_workspace_bytes(F32, 4, 32, 8, 12, 32) == 0
    assert lib.cgic_spatial_norm_workspace_bytes(F32, 1, 64, 136, 128, 32) == 32 * 65 * 8

    def refused(code, text, *args):
        with pytest.raises(cg.CgicError) as got:
            _lib.call("cgic_spatial_norm", *args)
        assert got.value.code == code and text in str(got.value), str(got.value)

    a = [BASE[k] for k in ORDER]
    f, zq, gw, gb, wy, by, wb, bb, out, ws = a
    refused(UNSUPPORTED, "zq 4x3 under features 6x6", f, F32, 1, 32, 6, 6, zq, 4, 3, 32, 1e-6, gw, gb, wy, by, wb, bb, 0, out, F32, ws, BIG, None)
    refused(UNSUPPORTED, PAIR % (1, 0), f, F32, 1, 32, 8, 12, zq, 2, 3, 32, 1e-6, gw, gb, wy, by, wb, bb, 0, out, F16, ws, BIG, None)
    refused(INVALID, OVERLAP, f, F16, 1, 32, 8, 12, zq, 2, 3, 32, 1e-6, gw, gb, wy, by, wb, bb, 1, f, F32, ws, BIG, None)
    refused(CAPACITY, WS % 0, f, F32, 3, 32, 8, 12, zq, 2, 3, 32, 1e-6, gw, gb, wy, by, wb, bb, 0, out, F32, None, 0, None)
    refused(INVALID, "spatial_norm: NULL tensor", f, F32, 1, 32, 8, 12, None, 2, 3, 32, 1e-6, gw, gb, wy, by, wb, bb, 0, out, F32, ws, BIG, None)
    refused(INVALID, "spatial_norm: eps -1", f, F32, 1, 32, 8, 12, zq, 2, 3, 32, -1.0, gw, gb, wy, by, wb, bb, 0, out, F32, ws, BIG, None)
    assert _lib.call("cgic_spatial_norm", None, F32, 0, 32, 8, 12, None, 2, 3, 32, 1e-6, None, None, None, None, None, None, 0, None, F32, None, 0, None) == OK
