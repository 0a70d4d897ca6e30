"""The launch plans of the tiled path (csrc/cgic_tiles_plan.h) without a GPU.
The plan header is plain C++17: tests/host/tiles_plan_main.cpp is compiled with the host compiler alone -- once plainly, once with
-fsanitize=address,undefined -- and run as a program over the table below, whose rows were worked out by hand:
  cut:        first[k] = running sum of (u8 ? 1 : 3) * th * (tw / 4), every sum a multiple of 64 and below 2^31;
              blocks = min(ceil(total / 256), 16384), grid (blocks, N)
  paste:      items = th * (tw / 4) of the largest tile; blocks = min(ceil(items / 256), 4096), grid (blocks, ntiles, N); stride4 = stride / 4
  partition:  items = th * ceil(tw / 4); masks form: sides multiples of 16, grid 0x0 or th/4 x tw/4; indices form: 1 <= gh <= th, 1 <= gw <= tw
  clip:       [max(y0, 0), min(y0 + th, H)) x [max(x0, 0), min(x0 + tw, W)); only non-empty clips can overlap
A row with several faults expects the first one in the order the entry points always checked; each such row restates a case that
tests/test_paste_host.py, tests/test_partition_host.py or tests/test_launch_groups.py pins through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2

# the six tiles of a 1356x2040 image (pad: 2 rows above, 4 columns left; padded 1360x2048 = rows 768 + 592, columns 768 + 768 + 512),
# row-major, origins in unpadded coordinates
SIX = " ".join(f"{y - 2} {x - 4} {th} {tw}" for y, th in ((0, 768), (768, 592)) for x, tw in ((0, 768), (768, 768), (1536, 512)))
F768, F512, G768, G512 = 3 * 768 * 192, 3 * 768 * 128, 3 * 592 * 192, 3 * 592 * 128          # fp32 items: 442368 294912 340992 227328

CASES = [
    # ---- clip and disjoint
    ("K -8 -8 16 16 16 16", dict(clip="0,8,0,8", empty="0")),
    ("K -16 0 16 16 16 16", dict(clip="0,0,0,16", empty="1")),
    ("K 8 8 16 16 16 16", dict(clip="8,16,8,16", empty="0")),
    ("D 32 32 2  0 0 16 16  0 16 16 16", dict(apart="1")),
    ("D 32 32 2  0 0 16 16  8 8 16 16", dict(apart="0", j="0", k="1")),
    ("D 32 32 3  0 0 16 16  16 16 16 16  8 8 16 16", dict(apart="0", j="0", k="2")),
    ("D 32 32 2  -16 -8 16 16  -16 -8 16 16", dict(apart="1")),                 # coincide wholly inside the pad: both clips empty
    # an overlap that lies only in the pad.  (With BOTH clips non-empty there is none: the intersection of two rectangles misses the
    # image only where it lies beyond one of the image's four edges, and then so does one of the two.)  One empty, one not:
    ("D 32 32 2  -16 0 16 16  -8 0 16 16", dict(apart="1")),
    ("D 32 32 2  -8 -8 16 16  -8 0 16 16", dict(apart="0", j="0", k="1")),      # share rows 0..8, columns 0..8 of the image
    # ---- cut, accepted
    ("C 0 1 16 16 1  0 0 16 16", dict(total="192", blocks="1", gy="1", first="0")),
    ("C 1 1 16 16 1  0 0 16 16", dict(total="64", blocks="1", first="0")),
    ("C 0 3 768 768 1  0 0 768 768", dict(total="442368", blocks="1728", gy="3")),
    (f"C 0 1 1356 2040 6  {SIX}", dict(total="2088960", blocks="8160",
                                       first=f"0,{F768},{2 * F768},{2 * F768 + F512},{2 * F768 + F512 + G768},{2 * F768 + F512 + 2 * G768}")),
    (f"C 1 1 1356 2040 6  {SIX}", dict(total=str(2088960 // 3), blocks="2720")),
    ("C 0 1 768 768 10  0 0 768 768", dict(total="4423680", blocks="16384")),  # ceil = 17280 workgroups: capped
    ("C 0 0 16 16 1  0 0 16 16", dict(total="192", gy="0")),                    # N = 0 plans; the entry point then launches nothing
    # ---- cut, refused
    ("C 1 1 16 16 1  0 0 8 16", dict(err=UNSUPPORTED, why="CUT_WAVE", k="0")),   # running sum 32
    ("C 1 1 16 32 2  0 0 16 16  0 16 8 16", dict(err=UNSUPPORTED, why="CUT_WAVE", k="1")),     # 64, then 96
    ("C 0 1 16 1600 97  0 0 16 16", dict(err=UNSUPPORTED, why="COUNT")),
    ("C 0 1 16 16 0", dict(err=UNSUPPORTED, why="COUNT")),
    ("C 0 1 16 16 1  0 0 16 6", dict(err=INVALID, why="TILE_SHAPE", k="0")),
    ("C 0 1 16 16 1  0 1073741824 16 16", dict(err=INVALID, why="ORIGIN")),
    ("C 0 65536 16 16 1  0 0 16 16", dict(err=UNSUPPORTED, why="IMAGES")),
    ("C 0 1 16 16 2  0 0 65536 43692  0 0 16 16", dict(err=UNSUPPORTED, why="CUT_TOO_LARGE", k="0")),      # 3 * 65536 * 10923 >= 2^31
    ("C 0 1 16 16 97  0 0 16 6", dict(err=UNSUPPORTED, why="COUNT")),           # the count before any tile (test_launch_groups)
    # ---- paste
    ("P 1 32 32 1  0 0 16 16 768 1", dict(most="64", blocks="1", gy="1", gz="1", stride4="192")),
    ("P 2 768 768 1  0 0 768 768 1769472 1", dict(most="147456", blocks="576", gz="2", stride4="442368")),
    ("P 1 4096 1024 1  0 0 4096 1024 768 0", dict(most="1048576", blocks="4096")),
    ("P 1 4097 1024 1  0 0 4097 1024 768 0", dict(most="1048832", blocks="4096")),           # ceil = 4097: capped
    ("P 5 32 64 3  0 0 16 16 768 1  0 16 32 32 3072 1  16 0 16 16 768 1", dict(most="256", blocks="1", gy="3", gz="5", stride4="192,768,192")),
    ("P 1 32 32 1  0 0 65536 16 768 1", dict(err=UNSUPPORTED, why="TILE_SIDE", k="0")),
    ("P 1 32 32 1  0 0 16 16 17179869184 1", dict(err=UNSUPPORTED, why="PASTE_STRIDE")),
    ("P 1 32 32 1  0 0 16 16 17179869180 1", dict(most="64", stride4="4294967295")),
    ("P 1 32 32 1  0 0 16 16 6 1", dict(err=INVALID, why="PASTE_SOURCE")),
    ("P 1 32 32 1  0 0 16 16 768 2", dict(err=INVALID, why="PASTE_WEIGHT_PAIR")),
    ("P 1 32 32 1  0 0 16 16 768 3", dict(err=INVALID, why="PASTE_WEIGHT_PAIR")),
    ("P 1 32 32 2  0 0 16 16 768 1  8 8 16 16 768 1", dict(err=UNSUPPORTED, why="OVERLAP", j="0", k="1")),
    ("P 1 32 1600 97  0 0 16 16 768 1", dict(err=UNSUPPORTED, why="COUNT")),
    ("P 1 32 1600 96  0 0 16 16 768 1", dict(most="64", gy="96")),
    ("P 65536 32 32 1  0 0 16 16 768 1", dict(err=UNSUPPORTED, why="IMAGES")),
    # ---- partition
    ("M 0 1 32 32 0 1  i 0 0 16 18 4 4", dict(masks="0", most="80", blocks="1", grid="4x4")),           # 5 items a row
    ("M 0 1 32 32 0 1  m 0 0 16 16 0 0", dict(masks="1", most="64", grid="4x4")),
    ("M 1 2 64 64 0 2  m 0 0 64 32 16 8  m 0 32 64 32 0 0", dict(masks="1", most="512", blocks="2", gy="2", gz="2", grid="16x8,16x8")),
    ("M 0 1 32 32 0 1  m 0 0 24 16 0 0", dict(err=INVALID, why="PARTITION_MASK_SIDES")),
    ("M 0 1 32 32 0 1  m 0 0 16 16 5 4", dict(err=INVALID, why="PARTITION_MASK_GRID")),
    ("M 0 1 32 32 0 1  i 0 0 16 16 17 4", dict(err=UNSUPPORTED, why="PARTITION_INDEX_CELL")),
    ("M 0 1 32 32 0 1  i 0 0 16 16 0 4", dict(err=INVALID, why="PARTITION_INDEX_GRID")),
    ("M 0 1 32 32 0 2  m 0 0 16 16 0 0  i 0 16 16 16 4 4", dict(err=INVALID, why="PARTITION_MIXED", k="1")),
    ("M 0 1 32 32 0 1  b 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_FORM")),
    ("M 0 1 32 32 0 1  n 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_FORM")),
    ("M 0 1 32 1600 0 85  m 0 0 16 16 0 0", dict(err=UNSUPPORTED, why="COUNT")),
    ("M 0 1 32 1600 0 84  m 0 0 16 16 0 0", dict(masks="1", gy="84")),
    ("M 0 1 32 32 0 2  m 0 0 16 16 0 0  m 8 8 16 16 0 0", dict(err=UNSUPPORTED, why="OVERLAP", j="0", k="1")),
    # the aliasing rule: an output may BE the source, in the source's layout
    ("M 0 1 32 32 1 1  m 0 0 16 16 0 0", dict(masks="1")),
    ("M 0 1 32 32 2 1  m 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_F32_ON_SRC")),
    ("M 1 1 32 32 1 1  m 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_F32_ON_SRC")),               # the address in another layout
    ("M 1 1 32 32 3 1  m 0 0 16 16 0 0", dict(masks="1")),
    ("M 0 1 32 32 3 1  m 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_U8_ON_SRC")),
    ("M 0 1 32 32 4 1  m 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_OUTPUTS")),
    # several faults: the image limits before the aliasing rule (test_partition_host: N = 65536 and W = 70000 with an out_f32 that
    # the source of that size would reach)
    ("M 0 65536 32 32 2 1  m 0 0 16 16 0 0", dict(err=UNSUPPORTED, why="IMAGES")),
    ("M 0 1 32 70000 2 1  m 0 0 16 16 0 0", dict(err=UNSUPPORTED, why="PARTITION_IMAGE_SIDE")),
    ("M 2 1 32 32 0 1  m 0 0 16 16 0 0", dict(err=INVALID, why="PARTITION_SRC_KIND")),
]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "tiles_plan_main.cpp"), "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], input="\n".join(c for c, _ in CASES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    return [dict(t.split("=", 1) for t in line.split()) for line in lines]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("tiles_plan"), [], "tiles_plan_main"))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}-" + c.split("  ")[0].replace(" ", "_")[:28] for k, (c, _) in enumerate(CASES)])
def test_tiles_plan(plans, k):
    want, got = dict(CASES[k][1]), plans[k]
    if "err" in want:
        want["err"] = str(want["err"])
    else:
        assert "err" not in got, got
    assert {key: got.get(key) for key in want} == want, got


def test_tiles_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported (the descriptor tables are exact-size
    heap blocks, so a read past the tile count would be seen)"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tiles_plan_main_san")
    assert _run(exe) == plans
