"""The launch plan of cgic_compress_streams (csrc/cgic_coder_plan.h) without a GPU: how the index streams are split into parts, the
staging in dynamic LDS, the tickets, the job count, which instantiation of the kernel and which grid order, and the sizes the size
queries answer.  The header is plain C++17: tests/host/coder_plan_main.cpp is compiled with the host compiler alone and run over the
table below, whose rows were worked out by hand from the arithmetic of the host path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_CAPACITY = 0, -1, -2, -5
K_LDS_POS = 8192

# max_len 20, 1024 symbols, a large slot, no histogram, a workspace unless a row says otherwise; h x w are latent grids
DEFAULTS = dict(slot=1 << 40, max_len=20, nsym=1024, hist=0, workspace=1)
FIELDS = ("B", "h", "w", "slot", "max_len", "nsym", "hist", "workspace")


def _case(name, B, h, w, want, **shape):
    return pytest.param(dict(DEFAULTS, B=B, h=h, w=w, **shape), want, id=name)


def _plan(parts, stage, dyn_lds, tickets, combine, jobs, small, parts_fastest, slot_need, ws_bytes=None):
    want = dict(parts_c=parts[0], parts_m=parts[1], parts_f=parts[2], stage=stage, dyn_lds=dyn_lds, tickets=tickets, combine=combine,
                jobs=jobs, small=small, parts_fastest=parts_fastest, slot_need=slot_need)
    if ws_bytes is not None:
        want["ws_bytes"] = ws_bytes
    return want


def _with_hist(case):
    """the same row with the usage histogram asked for: one job more per image, everything else as it was"""
    shape, want = case.values
    return pytest.param(dict(shape, hist=1), dict(want, jobs=want["jobs"] + 1), id=case.id + "-hist")


PLANS = [
    _case("64x64x64", 64, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 10256, 0)),
    _case("1x4x4", 1, 4, 4, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 64, 0)),
    _case("2x64x128", 2, 64, 128, _plan((1, 1, 1), 0, 0, 0, 1, 3, 0, 0, 20496, 0)),
    # the smallest split: 8448 fine positions in 3 parts of 2816
    _case("2x64x132", 2, 64, 132, _plan((1, 1, 3), 2816, 5696, 12, 0, 7, 0, 1, 21136, 304128)),
    _case("1x128x96", 1, 128, 96, _plan((1, 1, 3), 4096, 8256, 6, 0, 7, 0, 1, 30736, 221184)),
    _case("8x192x192", 8, 192, 192, _plan((1, 3, 7), 5268, 10608, 48, 0, 13, 0, 1, 92176, 5308416)),
    _case("1x256x256", 1, 256, 256, _plan((1, 4, 7), 9364, 18800, 6, 0, 14, 0, 1, 163856, 1179648)),
    _case("1x340x512", 1, 340, 512, _plan((3, 7, 7), 24872, 49808, 6, 0, 19, 0, 1, 435216, 3133440)),
    # 6 x 682 = 4092 slots: the last batch one ticket request covers
    _case("682x192x192", 682, 192, 192, _plan((1, 3, 7), 5268, 10608, 4092, 0, 13, 0, 1, 92176)),
    # beyond one ticket request: unsplit, the whole fine stream staged
    _case("683x192x192", 683, 192, 192, _plan((1, 1, 1), 36864, 73792, 0, 0, 5, 0, 0, 92176)),
    # unsplit and no staging room (65536 positions x 2 bytes > 96 KB): round by round through the workspace
    _case("700x256x256", 700, 256, 256, _plan((1, 1, 1), 0, 0, 0, 0, 5, 0, 0, 163856)),
    # split, but a part of the fine stream (7 x 84 264 positions) exceeds the 96 KB stage: the parts are reset
    _case("1x768x768", 1, 768, 768, _plan((1, 1, 1), 0, 0, 0, 0, 5, 0, 0, 1474576, 10616832)),
    # no workspace is needed up to kLdsPos positions
    _case("2x64x128-no-workspace", 2, 64, 128, _plan((1, 1, 1), 0, 0, 0, 1, 3, 0, 0, 20496, 0), workspace=0),
    _case("64x64x64-slot-exact", 64, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 10256, 0), slot=10256),
]
PLANS += [_with_hist(c) for c in PLANS]
PLANS += [
    # a histogram of more bins than the small instantiation's LDS arrays hold: the kLdsPos instantiation
    _case("1x64x64-hist-nsym8192", 1, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 4, 0, 0, 10256, 0), hist=1, nsym=8192),
    _case("1x64x64-hist-nsym4096", 1, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 4, 1, 0, 10256, 0), hist=1, nsym=4096),
    # an empty batch asks for nothing, and is answered before the histogram's bound is looked at
    _case("0x64x64-hist-nsym8193", 0, 64, 64, dict(jobs=0, tickets=0, dyn_lds=0), hist=1, nsym=8193),
]
# ---- a 64-bit code table (tests/test_long_codes.py): one row per form of the encoder, at the smallest grid (and batch) that reaches
# it, then the other shapes that file runs.  A slot is 8 h w + 10 bytes, rounded up to 16
LONG = dict(max_len=64)
PLANS += [
    # up to kLdsPosSmall positions: the small instantiation, the short jobs of an image in one workgroup
    _case("form-lds-small-1x64x64-l64", 1, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 32784, 0), **LONG),
    # up to kLdsPos positions: the same, the kLdsPos instantiation
    _case("form-lds-1x64x96-l64", 1, 64, 96, _plan((1, 1, 1), 0, 0, 0, 1, 3, 0, 0, 49168, 0), **LONG),
    # 8448 fine positions in 3 parts of 2816, each staged in 2 x 2816 + 64 bytes
    _case("form-parts-1x64x132-l64", 1, 64, 132, _plan((1, 1, 3), 2816, 5696, 6, 0, 7, 0, 1, 67600, 152064), **LONG),
    # 6 x 683 slots are beyond one ticket request: unsplit, all 8448 positions staged (2 x 8448 + 64 bytes)
    _case("form-staged-683x64x132-l64", 683, 64, 132, _plan((1, 1, 1), 8448, 16960, 0, 0, 5, 0, 0, 67600), **LONG),
    # 345 744 fine positions in 7 parts of 49 392: 98 784 bytes exceed the 96 KB stage: unsplit, round by round through the workspace
    _case("form-global-1x588x588-l64", 1, 588, 588, _plan((1, 1, 1), 0, 0, 0, 0, 5, 0, 0, 2765968, 6223392), **LONG),
    _case("3x64x64-l64", 3, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 32784, 0), **LONG),
    _case("40x64x64-l64", 40, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 32784, 0), **LONG),
    _case("1x4x4-l64", 1, 4, 4, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 144, 0), **LONG),
    _case("1x8x12-l64", 1, 8, 12, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 784, 0), **LONG),
    # 9216 fine positions in 3 parts of 3072
    _case("1x96x96-l64", 1, 96, 96, _plan((1, 1, 3), 3072, 6208, 6, 0, 7, 0, 1, 73744, 165888), **LONG),
    _case("12x96x96-l64", 12, 96, 96, _plan((1, 1, 3), 3072, 6208, 72, 0, 7, 0, 1, 73744, 1990656), **LONG),
    _case("1x72x116-l64", 1, 72, 116, _plan((1, 1, 3), 2784, 5632, 6, 0, 7, 0, 1, 66832, 150336), **LONG),
    _case("2x128x128-l64", 2, 128, 128, _plan((1, 1, 4), 4096, 8256, 12, 0, 8, 0, 1, 131088, 589824), **LONG),
    # 65 bits and three-word codes change the slot alone (65 x 4096 / 8 + 10), 2560 symbols nothing
    _case("1x64x64-l65", 1, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 33296, 0), max_len=65),
    _case("3x32x48-l65", 3, 32, 48, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 12496, 0), max_len=65),
    _case("3x64x64-l64-nsym2560", 3, 64, 64, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 32784, 0), nsym=2560, **LONG),
    _case("3x32x48-l33-nsym96", 3, 32, 48, _plan((1, 1, 1), 0, 0, 0, 1, 3, 1, 0, 6352, 0), max_len=33, nsym=96),
]
REFUSALS = [
    _case("slot-one-below", 64, 64, 64, dict(err=ERR_CAPACITY, why="slot=10255, need a multiple of 16 >= 10256"), slot=10255),
    _case("slot-16-below", 64, 64, 64, dict(err=ERR_CAPACITY, why="slot=10240, need a multiple of 16 >= 10256"), slot=10240),
    _case("slot-not-multiple-of-16", 64, 64, 64, dict(err=ERR_CAPACITY, why="slot=10264, need a multiple of 16 >= 10256"), slot=10264),
    _case("nsym-65537", 1, 64, 64, dict(err=ERR_UNSUPPORTED, why="table too large"), nsym=65537),
    # 128 bits x 2^25 positions = 2^32 bits
    _case("stream-2^32-bits", 1, 4096, 8192, dict(err=ERR_UNSUPPORTED, why="a stream could exceed 2^32 bits"), max_len=128),
    _case("2x64x132-no-workspace", 2, 64, 132, dict(err=ERR_INVALID, why="workspace required for 64x132 grids"), workspace=0),
    _case("hist-nsym8193", 1, 64, 64, dict(err=ERR_UNSUPPORTED, why="hist needs n <= 8192"), hist=1, nsym=8193),
    # the order of the checks: the slot before the table, the workspace before the histogram's bound
    _case("slot-before-table", 1, 64, 64, dict(err=ERR_CAPACITY, why="slot=16"), slot=16, nsym=65537),
    _case("workspace-before-hist", 2, 64, 132, dict(err=ERR_INVALID, why="workspace required"), workspace=0, hist=1, nsym=8193),
]
CASES = PLANS + REFUSALS


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every case of the table through ONE run of the compiled program: {case id: parsed output line}"""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp_path_factory.mktemp("coder_plan") / "coder_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", os.path.join(ROOT, "tests", "host", "coder_plan_main.cpp"), "-o", exe])
    text = "\n".join(" ".join(str(c.values[0][f]) for f in FIELDS) for c in CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    parsed = {}
    for c, line in zip(CASES, out):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            parsed[c.id] = {k: int(v) for k, v in (t.split("=", 1) for t in line.split())}
    return parsed


@pytest.mark.parametrize("shape,want", CASES)
def test_compress_plan(plans, request, shape, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got.get("err") == want["err"] and want["why"] in got["why"], got
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want
    B, h, w = shape["B"], shape["h"], shape["w"]
    parts = (got["parts_c"], got["parts_m"], got["parts_f"])
    assert (got["tickets"] == 0) == (parts == (1, 1, 1)) and got["tickets"] in (0, 6 * B)
    assert got["parts_fastest"] == (got["tickets"] != 0)
    assert not got["combine"] or h * w <= K_LDS_POS
    assert (got["dyn_lds"] == 0) == (got["stage"] == 0) and got["dyn_lds"] % 16 == 0 and got["dyn_lds"] >= 2 * got["stage"]
    if B:
        assert got["recorded"] == (not got["small"]) and (not got["small"] or got["combine"])
        assert got["jobs"] == (3 if got["combine"] else sum(parts) + 2) + shape["hist"]
    # a part covers whole groups of four positions, and the parts together every position
    for name, sh, P in zip("cmf", (2, 1, 0), parts):
        npos, per = (h >> sh) * (w >> sh), got["per_" + name]
        assert per * P >= npos and per % 4 == 0
        assert P == 1 or per <= got["stage"]          # every part of a split stream fits the stage
    # the sizes: the workspace holds a u32 and a u16 per reserved position, the symbols behind the end bits
    assert got["ws_stride"] % 8 == 0 and 0 <= got["ws_stride"] - h * w < 8
    assert got["ws_sym_offset"] == B * 3 * got["ws_stride"] * 4
    assert got["ws_bytes"] == (B * 3 * got["ws_stride"] * 6 if h * w > K_LDS_POS else 0)
    assert got["slot_need"] == max(got["capacity"], (((h // 2) * (w // 2) // 8 + 2 + 8) + 15) // 16 * 16)
    assert got["capacity"] == ((shape["max_len"] * h * w // 8 + 2 + 8) + 15) // 16 * 16
    assert got["stream_ws"] == ((h * w * 4 + 15) // 16 * 16 + (h * w * 2 + 15) // 16 * 16 if h * w > K_LDS_POS else 0)
