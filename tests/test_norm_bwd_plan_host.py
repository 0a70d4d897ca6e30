"""The launch plans of cgic_spatial_norm_backward and cgic_spatial_norm_train (csrc/cgic_norm_bwd_plan.h) without a GPU: every check
of the call, the unit, the layout of the workspace and the three grids.  tests/host/norm_bwd_plan_main.cpp is compiled with the host
compiler alone -- once plainly, once with -fsanitize=address,undefined -- and run as a program over the table below, whose rows were
worked out by hand:
  chan_block = 32, halved (down to 8) while ceil(C / chan_block) * ceil(H * W / 1024) < 64;  chan_blocks = ceil(C / chan_block);
  tiles_max = ceil(H * W / 256);  workspace = B * C * tiles_max * 96  (the twelve float64 sums per (b, c, tile), at off_sums = 0)
      + B * C * 16  (off_span)  + B * chan_blocks * 4 * H * W * 4  (off_dz): a function of the shape alone;
  unit = the largest of 8 (halves only), 4, 2 that divides W and whose access (unit elements, 16 bytes at most) f, go and df (where
      wanted) are aligned to; else 1;
  threads_reduce = 64 / 128 / 256 for H * W / unit <= 64 / <= 128 / more;  tiles = ceil(H * W / unit / threads_reduce);
  grid_reduce = B * chan_blocks * tiles;  grid_sums = ceil(C * 12 / 256);  grid_dzq = ceil(B * 4 * hq * wq / 256), 0 without dzq;
  parts = ceil(H * W / unit / 1024), grid_apply = min(B * C * parts, 16384), both 0 without df;
  need_dz: dzq is wanted; need_conv: any of dwy, dby, dwb, dbb is (otherwise reduce adds two sums per channel, not twelve); need_df;
  the nearest index, the magic multipliers and zq_vec as in the forward's plan (tests/test_norm_plan_host.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -5
F32, F16, BF16 = 0, 1, 2
IN = ("f", "go", "zq", "stats", "gn_weight", "gn_bias", "wy", "by", "wb", "bb")
OUT = ("df", "dzq", "dgn_weight", "dgn_bias", "dwy", "dby", "dwb", "dbb")
ORDER = IN + OUT + ("ws",)
BASE = {k: (i + 1) << 32 for i, k in enumerate(ORDER)}          # 4 GiB apart
BIG = 1 << 30
OVERLAP = "spatial_norm_backward: an output overlaps another tensor of the call (only df == go with equal types may)"
PAIR = "spatial_norm_backward: %s %d with in_dtype %d (CGIC_DT_F32 or the features' own type)"


def addresses(order, addr):
    a = {k: BASE[k] if k in BASE else TRAIN_BASE[k] for k in order}
    for key, v in addr.items():
        a[key] = v[1] if isinstance(v, tuple) else a[key] + v
    return a


def case(name, want, dt, dt_go, dt_df, B, C, H, W, hq, wq, groups=32, ws_bytes=BIG, **addr):
    """addr: f=+8 style byte offsets from the tensor's base, or absolute addresses as ("abs", value)"""
    a = addresses(ORDER, addr)
    line = " ".join(str(v) for v in (0, dt, dt_go, dt_df, B, C, H, W, hq, wq, groups, *(a[key] for key in ORDER), ws_bytes))
    return pytest.param(line, want, id=name)


TRAIN_ORDER = ("f", "zq", "gn_weight", "gn_bias", "wy", "by", "wb", "bb", "out", "ws")
TRAIN_BASE = {"out": 30 << 32, "tstats": 31 << 32}


def train(name, want, dt, dt_out, B, C, H, W, hq, wq, groups=32, ws_bytes=BIG, **addr):
    a = addresses(TRAIN_ORDER + ("tstats",), addr)
    line = " ".join(str(v) for v in (1, dt, dt_out, B, C, H, W, hq, wq, groups, *(a[key] for key in TRAIN_ORDER), ws_bytes, a["tstats"]))
    return pytest.param(line, want, id=name)


def plan(unit, B, C, H, W, hq, wq, chan_block, threads, tiles, groups=32, dzq=True, df=True, **kw):
    plane = H * W
    blocks = -(-C // chan_block)
    tiles_max = -(-plane // 256)
    off_span = B * C * tiles_max * 96
    off_dz = off_span + B * C * 16
    parts = -(-(plane // unit) // 1024)
    return dict(unit=unit, span=C // groups * plane, spans=B * groups, chan_block=chan_block, chan_blocks=blocks, threads_reduce=threads, tiles=tiles,
                tiles_max=tiles_max, grid_reduce=B * blocks * tiles, grid_sums=-(-C * 12 // 256), grid_dzq=-(-B * 4 * hq * wq // 256) if dzq else 0,
                need_dz=int(dzq), parts=parts if df else 0, grid_apply=min(B * C * parts, 16384) if df else 0, off_sums=0, off_span=off_span,
                off_dz=off_dz, workspace=off_dz + B * blocks * 4 * plane * 4, **kw)


def err(code, why):
    return dict(err=code, why=why)


GO = BASE["go"]
NULLS = {k: ("abs", 0) for k in ORDER}
NO_PARAMS = {k: ("abs", 0) for k in OUT[2:]}
CASES = [
    # ---- the channel block, the tile and the workspace by the shape (hand-worked: see the module docstring)
    # [4,64,6,10]: 2 * 1 < 64 -> 16: 4 -> 8: 8 blocks; 60 pixels: one tile of 64 threads at unit 2 (30 units); 24576 + 4096 + 30720
    case("4x64x6x10", {**plan(2, 4, 64, 6, 10, 12, 5, 8, 64, 1, ymul=2, ydiv=1, xmul=1, xdiv=2, zq_vec=0, in_place=0), "workspace": 59392},
         F32, F32, F32, 4, 64, 6, 10, 12, 5),
    # [1,64,136,128]: 17408 pixels = 17 k-pixel tiles: 2 * 17 < 64 -> 16: 4 * 17 = 68; unit 4: 4352 units = 17 tiles of 256; tiles_max 68
    case("1x64x136x128", {**plan(4, 1, 64, 136, 128, 34, 32, 16, 256, 17, ydiv=4, xdiv=4), "tiles_max": 68, "grid_reduce": 68, "parts": 5,
                          "grid_apply": 320, "workspace": 64 * 68 * 96 + 64 * 16 + 4 * 4 * 17408 * 4},
         F32, F32, F32, 1, 64, 136, 128, 34, 32),
    # [2,128,256,256] fp16: 4 * 64 >= 64 -> 32; unit 8: 8192 units = 32 tiles
    case("2x128x256x256-f16", plan(8, 2, 128, 256, 256, 64, 64, 32, 256, 32, ydiv=4, xdiv=4), F16, F32, F16, 2, 128, 256, 256, 64, 64),
    # [4,512,16,16]: 16 * 1 < 64 -> 16: 32 -> 8: 64 blocks; 256 pixels at unit 4: 64 units, 64 threads
    case("4x512x16x16-down4", plan(4, 4, 512, 16, 16, 64, 64, 8, 64, 1, ymul=4, xmul=4, ydiv=1, xdiv=1, zq_vec=0), F32, F32, F32, 4, 512, 16, 16, 64, 64),
    case("1x32x34x68", plan(4, 1, 32, 34, 68, 17, 17, 8, 256, 3, ydiv=2, xdiv=4), F32, F32, F32, 1, 32, 34, 68, 17, 17),
    case("threads-128", plan(1, 1, 32, 5, 25, 5, 25, 8, 128, 1, zq_vec=1), F32, F32, F32, 1, 32, 5, 25, 5, 25),
    case("threads-64-at-64-units", plan(4, 1, 32, 16, 16, 16, 16, 8, 64, 1), F32, F32, F32, 1, 32, 16, 16, 16, 16),
    case("threads-128-at-65-units", plan(1, 1, 32, 5, 13, 5, 13, 8, 128, 1), F32, F32, F32, 1, 32, 5, 13, 5, 13),
    case("threads-256-at-129-units", plan(1, 1, 32, 3, 43, 3, 43, 8, 256, 1), F32, F32, F32, 1, 32, 3, 43, 3, 43),
    case("groups-16", plan(4, 1, 32, 8, 12, 2, 3, 8, 64, 1, groups=16), F32, F32, F32, 1, 32, 8, 12, 2, 3, groups=16),
    # ---- the outputs that are wanted
    case("df-only", plan(2, 4, 64, 6, 10, 12, 5, 8, 64, 1, dzq=False, need_conv=0, need_df=1), F32, F32, F32, 4, 64, 6, 10, 12, 5, dzq=("abs", 0), **NO_PARAMS),
    case("all-but-df", plan(2, 4, 64, 6, 10, 12, 5, 8, 64, 1, df=False, need_conv=1, need_df=0), F32, F32, F32, 4, 64, 6, 10, 12, 5, df=("abs", 0)),
    case("dgn_bias-only", plan(2, 4, 64, 6, 10, 12, 5, 8, 64, 1, df=False, dzq=False, need_conv=0, need_df=0), F32, F32, F32, 4, 64, 6, 10, 12, 5,
         **{**{k: ("abs", 0) for k in OUT}, "dgn_bias": 0}),
    case("dbb-only", plan(2, 4, 64, 6, 10, 12, 5, 8, 64, 1, df=False, dzq=False, need_conv=1, need_df=0), F32, F32, F32, 4, 64, 6, 10, 12, 5,
         **{**{k: ("abs", 0) for k in OUT}, "dbb": 0}),
    case("nothing-wanted", err(INVALID, "spatial_norm_backward: no gradient is wanted (every output is NULL)"), F32, F32, F32, 4, 64, 6, 10, 12, 5,
         **{k: ("abs", 0) for k in OUT}),
    # ---- the magic multipliers and zq_vec: 2^32 / 12 = 357913941.3, / 4 = 1073741824
    case("magic-8x12-up4", plan(4, 4, 32, 8, 12, 2, 3, 8, 64, 1, mg_w=357913942, mg_y=1073741824, mg_x=1073741824, zq_vec=0), F32, F32, F32, 4, 32, 8, 12, 2, 3),
    case("zq_vec", plan(4, 1, 32, 12, 12, 4, 12, 8, 64, 1, mg_x=0, zq_vec=1), F32, F32, F32, 1, 32, 12, 12, 4, 12),
    case("zq+4-no-zq_vec", plan(4, 1, 32, 12, 12, 4, 12, 8, 64, 1, zq_vec=0), F32, F32, F32, 1, 32, 12, 12, 4, 12, zq=4),
]
# ---- the unit by row width (aligned pointers), [1,32,2,W] on zq [1,4,2,W]
for dt, w, unit in ((F32, 2, 2), (F32, 3, 1), (F32, 4, 4), (F32, 6, 2), (F16, 8, 8), (F16, 12, 4), (F16, 10, 2), (BF16, 5, 1), (BF16, 16, 8)):
    CASES.append(case(f"unit-dt{dt}-w{w}", plan(unit, 1, 32, 2, w, 2, w, 8, 64, 1), dt, dt, dt, 1, 32, 2, w, 2, w))
# ---- the unit by pointer alignment: halves on [1,32,2,16]; go and df in fp32 (dt 0) or the half type
for name, unit, dt_go, dt_df, addr in (("f+2", 1, F32, F32, dict(f=2)), ("f+4", 2, F32, F32, dict(f=4)), ("f+8", 4, F32, F32, dict(f=8)), ("f+16", 8, F32, F32, dict(f=16)),
                                       ("go32+4", 1, F32, F32, dict(go=4)), ("go32+8", 2, F32, F32, dict(go=8)), ("go32+16", 8, F32, F32, dict(go=16)),
                                       ("go16+2", 1, F16, F32, dict(go=2)), ("go16+8", 4, F16, F32, dict(go=8)),
                                       ("df32+8", 2, F32, F32, dict(df=8)), ("df16+4", 2, F32, F16, dict(df=4)), ("df16+16", 8, F32, F16, dict(df=16)),
                                       ("df+2-not-wanted", 8, F32, F16, dict(df=("abs", 0))),
                                       ("dzq+4-does-not-matter", 8, F32, F32, dict(dzq=4)), ("stats+4-does-not-matter", 8, F32, F32, dict(stats=4))):
    CASES.append(case(f"align-{name}", dict(unit=unit), F16, dt_go, dt_df, 1, 32, 2, 16, 2, 16, **addr))
ALIGN = "spatial_norm_backward: a pointer is not aligned to its %d-byte element"
CASES += [
    case("misaligned-f16+1", err(INVALID, ALIGN % 2), F16, F32, F32, 1, 32, 2, 16, 2, 16, f=1),
    case("misaligned-go32+2", err(INVALID, ALIGN % 4), F16, F32, F32, 1, 32, 2, 16, 2, 16, go=2),
    case("misaligned-go16+1", err(INVALID, ALIGN % 2), F16, F16, F32, 1, 32, 2, 16, 2, 16, go=1),
    case("misaligned-stats+2", err(INVALID, ALIGN % 4), F32, F32, F32, 1, 32, 2, 16, 2, 16, stats=2),
    case("misaligned-df16+1", err(INVALID, ALIGN % 2), F16, F32, F16, 1, 32, 2, 16, 2, 16, df=1),
    case("misaligned-dwb+2", err(INVALID, ALIGN % 4), F32, F32, F32, 1, 32, 2, 16, 2, 16, dwb=2),
]
# ---- the types
for dt, dt_go, dt_df in ((F32, F32, F32), (F16, F32, F32), (F16, F16, F32), (F16, F32, F16), (F16, F16, F16), (BF16, BF16, BF16), (BF16, F32, BF16)):
    CASES.append(case(f"types-{dt}{dt_go}{dt_df}", dict(unit=4 if dt == F32 else 8), dt, dt_go, dt_df, 1, 32, 2, 16, 2, 16))
CASES += [
    case("types-go16-on-f32", err(UNSUPPORTED, PAIR % ("go_dtype", 1, 0)), F32, F16, F32, 1, 32, 2, 16, 2, 16),
    case("types-df-bf16-on-f16", err(UNSUPPORTED, PAIR % ("df_dtype", 2, 1)), F16, F16, BF16, 1, 32, 2, 16, 2, 16),
    case("types-go-before-df", err(UNSUPPORTED, PAIR % ("go_dtype", 2, 1)), F16, BF16, BF16, 1, 32, 2, 16, 2, 16),
    case("types-df-7", err(INVALID, PAIR % ("df_dtype", 7, 1)), F16, F16, 7, 1, 32, 2, 16, 2, 16),
    case("types-in-3", err(INVALID, "spatial_norm: in_dtype 3 (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)"), 3, F32, F32, 1, 32, 2, 16, 2, 16),
]
# ---- the shapes, in the order of the checks
RATIO = "spatial_norm_backward: zq %dx%d under features %dx%d (each axis an integer ratio, up or down)"
CASES += [
    case("B-1", err(INVALID, "spatial_norm: features [-1,32,8,12]"), F32, F32, F32, -1, 32, 8, 12, 2, 3),
    case("B0", err(INVALID, "spatial_norm_backward: an empty batch"), F32, F32, F32, 0, 32, 8, 12, 2, 3),
    case("48-in-32", err(INVALID, "spatial_norm: 48 channels in 32 groups"), F32, F32, F32, 1, 48, 8, 12, 2, 3),
    case("beyond-2^31", err(UNSUPPORTED, "spatial_norm: a group of 1 x 65536x65536 elements is beyond 2^31"), F32, F32, F32, 1, 32, 65536, 65536, 1, 1),
    case("grid-beyond-2^31", err(UNSUPPORTED, "spatial_norm_backward: [131072,32,2048,2048] is beyond a grid of 2^31 workgroups"),
         F32, F32, F32, 131072, 32, 2048, 2048, 1, 1),
    case("zq-0x3", err(INVALID, "spatial_norm_backward: zq grid 0x3"), F32, F32, F32, 1, 32, 8, 12, 0, 3),
    case("ratio-6-over-4", err(UNSUPPORTED, RATIO % (4, 3, 6, 6)), F32, F32, F32, 1, 32, 6, 6, 4, 3),
    case("ratio-x-4-over-6", err(UNSUPPORTED, RATIO % (2, 6, 4, 4)), F32, F32, F32, 1, 32, 4, 4, 2, 6),
    case("types-before-zq", err(UNSUPPORTED, PAIR % ("go_dtype", 1, 0)), F32, F16, F32, 1, 32, 6, 6, 4, 3),
    case("NULL-all", err(INVALID, "spatial_norm_backward: NULL input"), F32, F32, F32, 1, 32, 8, 12, 2, 3, **NULLS),
    case("NULL-stats", err(INVALID, "spatial_norm_backward: NULL input"), F32, F32, F32, 1, 32, 8, 12, 2, 3, stats=("abs", 0)),
    case("NULL-go", err(INVALID, "spatial_norm_backward: NULL input"), F32, F32, F32, 1, 32, 8, 12, 2, 3, go=("abs", 0)),
]
# ---- aliasing: [1,32,8,12] = 3072 elements, 12288 bytes of fp32
CASES += [
    case("df-on-go-f32", dict(unit=4, in_place=1), F32, F32, F32, 1, 32, 8, 12, 2, 3, df=("abs", GO)),
    case("df-on-go-f16", dict(unit=4, in_place=1), F16, F16, F16, 1, 32, 8, 12, 2, 3, df=("abs", GO)),
    case("f32-df-on-f16-go", err(INVALID, OVERLAP), F16, F16, F32, 1, 32, 8, 12, 2, 3, df=("abs", GO)),
    case("f16-df-on-f32-go", err(INVALID, OVERLAP), F16, F32, F16, 1, 32, 8, 12, 2, 3, df=("abs", GO)),
    case("df-inside-go", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, df=("abs", GO + 16)),
    case("df-on-f", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, df=("abs", BASE["f"])),
    case("df-ends-inside-f", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, df=("abs", BASE["f"] - 12288 + 16)),
    case("df-before-f", dict(unit=4, in_place=0), F32, F32, F32, 1, 32, 8, 12, 2, 3, df=("abs", BASE["f"] - 12288)),
    case("dzq-on-zq", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, dzq=("abs", BASE["zq"])),
    case("dwy-on-wy", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, dwy=("abs", BASE["wy"])),
    case("dby-on-stats", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, dby=("abs", BASE["stats"] + 128)),
    case("dgn_bias-on-dgn_weight", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, dgn_bias=("abs", BASE["dgn_weight"] + 64)),
    case("dbb-behind-dwb", dict(unit=4), F32, F32, F32, 1, 32, 8, 12, 2, 3, dbb=("abs", BASE["dwb"] + 512)),
    case("dbb-on-the-end-of-dwb", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, dbb=("abs", BASE["dwb"] + 508)),
    case("dzq-on-go-may-not", err(INVALID, OVERLAP), F32, F32, F32, 1, 32, 8, 12, 2, 3, dzq=("abs", GO)),
]
# ---- the workspace: [3,32,8,12]: 3 * 32 * 1 * 96 + 3 * 32 * 16 + 3 * 4 * 4 * 96 * 4 = 9216 + 1536 + 18432 = 29184 bytes
WS = "spatial_norm_backward: workspace of %d bytes, need 29184 (cgic_spatial_norm_backward_workspace_bytes)"
WS_CLASH = "spatial_norm_backward: the workspace overlaps a tensor of the call"
CASES += [
    case("ws-exact", dict(workspace=29184, off_span=9216, off_dz=10752, chan_block=8, chan_blocks=4), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws_bytes=29184),
    case("ws-one-short", err(CAPACITY, WS % 29183), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws_bytes=29183),
    case("ws-NULL", err(CAPACITY, WS % 0), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", 0)),
    case("ws+8", err(INVALID, "spatial_norm_backward: the workspace is not aligned to 16 bytes"), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws=8),
    case("ws-on-df", err(INVALID, WS_CLASH), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", BASE["df"] + 64)),
    case("ws-ends-in-f", err(INVALID, WS_CLASH), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", BASE["f"] - 29168)),
    case("ws-on-dbb", err(INVALID, WS_CLASH), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", BASE["dbb"] - 16)),
    case("ws-before-f", dict(workspace=29184), F32, F32, F32, 3, 32, 8, 12, 2, 3, ws=("abs", BASE["f"] - 29184)),
    case("ws-on-an-output-that-is-not-wanted", dict(workspace=29184, need_dz=0), F32, F32, F32, 3, 32, 8, 12, 2, 3, dzq=("abs", 0), ws=("abs", BASE["dzq"])),
]
# ---- the training forward: the forward's plan (tests/test_norm_plan_host.py) and the statistics' tensor; [3,32,8,12]: 96 spans, two
# launches, 2304 bytes of workspace, 768 bytes of statistics
ST = TRAIN_BASE["tstats"]
CASES += [
    train("train-two-launches", dict(form=2, unit=4, spans=96, workspace=2304), F32, F32, 3, 32, 8, 12, 2, 3),
    train("train-one-launch", dict(form=1, unit=4, spans=128, workspace=0), F32, F32, 4, 32, 8, 12, 2, 3),
    train("train-empty-batch-NULL", dict(form=0, spans=0), F32, F32, 0, 32, 8, 12, 2, 3, ws_bytes=0, **{k: ("abs", 0) for k in TRAIN_ORDER + ("tstats",)}),
    train("train-stats-NULL", err(INVALID, "spatial_norm_train: stats is NULL"), F32, F32, 3, 32, 8, 12, 2, 3, tstats=("abs", 0)),
    train("train-stats+2", err(INVALID, "spatial_norm_train: stats is not aligned to its 4-byte element"), F32, F32, 3, 32, 8, 12, 2, 3, tstats=2),
    train("train-stats+4", dict(form=2), F32, F32, 3, 32, 8, 12, 2, 3, tstats=4),
    train("train-stats-on-out", err(INVALID, "spatial_norm_train: stats overlaps another tensor of the call"), F32, F32, 3, 32, 8, 12, 2, 3,
          tstats=("abs", TRAIN_BASE["out"] + 64)),
    train("train-stats-ends-in-f", err(INVALID, "spatial_norm_train: stats overlaps another tensor of the call"), F32, F32, 3, 32, 8, 12, 2, 3,
          tstats=("abs", BASE["f"] - 764)),
    train("train-stats-before-f", dict(form=2), F32, F32, 3, 32, 8, 12, 2, 3, tstats=("abs", BASE["f"] - 768)),
    train("train-stats-on-the-workspace", err(INVALID, "spatial_norm_train: stats overlaps another tensor of the call"), F32, F32, 3, 32, 8, 12, 2, 3,
          tstats=("abs", BASE["ws"] + 2300)),
    train("train-stats-behind-the-workspace", dict(form=2), F32, F32, 3, 32, 8, 12, 2, 3, tstats=("abs", BASE["ws"] + 2304)),
    train("train-one-launch-has-no-workspace-to-clash-with", dict(form=1), F32, F32, 4, 32, 8, 12, 2, 3, tstats=("abs", BASE["ws"])),
    train("train-the-forwards-refusals-first", err(UNSUPPORTED, "spatial_norm: zq 4x3 under features 6x6 (each axis an integer ratio, up or down)"),
          F32, F32, 1, 32, 6, 6, 4, 3, tstats=("abs", 0)),
]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "norm_bwd_plan_main.cpp"), "-o", exe])
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
    return _run(_build(tmp_path_factory.mktemp("norm_bwd_plan"), [], "norm_bwd_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_norm_bwd_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_norm_bwd_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "norm_bwd_plan_main_san")
    assert _run(exe) == plans


def test_the_library_answers_as_the_plan_does():
    """cgic_spatial_norm_backward_workspace_bytes is the plan's shape part, and a refused call enqueues nothing: it can be made without
    a device, with made-up addresses (never dereferenced)"""
    import control_gic_amd as cg
    from control_gic_amd import _lib
    lib = _lib.lib()
    size = lib.cgic_spatial_norm_backward_workspace_bytes
    assert size(F32, 3, 32, 8, 12, 32) == 29184 and size(F16, 3, 32, 8, 12, 32) == 29184 and size(F32, 4, 64, 6, 10, 32) == 59392
    assert size(F32, 1, 64, 136, 128, 32) == 64 * 68 * 96 + 64 * 16 + 4 * 4 * 17408 * 4
    assert size(F32, 1, 48, 8, 12, 32) == 0 and size(F32, 0, 32, 8, 12, 32) == 0 and size(5, 1, 32, 8, 12, 32) == 0

    def refused(name, code, text, *args):
        with pytest.raises(cg.CgicError) as got:
            _lib.call(name, *args)
        assert got.value.code == code and text in str(got.value), str(got.value)

    a = {k: BASE[k] for k in ORDER}
    ins = [a[k] for k in IN[2:]]
    outs = [a[k] for k in OUT[1:]]
    bwd = lambda **kw: (kw.get("f", a["f"]), kw.get("dt", F32), kw.get("go", a["go"]), kw.get("dt_go", F32), kw.get("B", 3), 32, 8, 12, ins[0],
                        kw.get("hq", 2), 3, 32, *ins[1:], 1, kw.get("df", a["df"]), kw.get("dt_df", F32), *outs, kw.get("ws", a["ws"]),
                        kw.get("ws_bytes", BIG), None)
    refused("cgic_spatial_norm_backward", UNSUPPORTED, RATIO % (5, 3, 8, 12), *bwd(hq=5))
    refused("cgic_spatial_norm_backward", UNSUPPORTED, PAIR % ("go_dtype", 1, 0), *bwd(dt_go=F16))
    refused("cgic_spatial_norm_backward", INVALID, OVERLAP, *bwd(df=a["f"]))
    refused("cgic_spatial_norm_backward", INVALID, OVERLAP, *bwd(dt=F16, dt_go=F16, df=a["go"]))
    refused("cgic_spatial_norm_backward", CAPACITY, WS % 0, *bwd(ws=None, ws_bytes=0))
    refused("cgic_spatial_norm_backward", CAPACITY, WS % 100, *bwd(ws_bytes=100))
    refused("cgic_spatial_norm_backward", INVALID, "spatial_norm_backward: an empty batch", *bwd(B=0))
    refused("cgic_spatial_norm_backward", INVALID, "spatial_norm_backward: NULL input", *bwd(go=None))
    fwd = [a["f"], F32, 3, 32, 8, 12, a["zq"], 2, 3, 32, 1e-6, *(a[k] for k in IN[4:]), 0, a["df"], F32]
    refused("cgic_spatial_norm_train", INVALID, "spatial_norm_train: stats is NULL", *fwd, None, a["ws"], BIG, None)
    refused("cgic_spatial_norm_train", INVALID, "spatial_norm_train: stats overlaps another tensor of the call", *fwd, a["df"] + 16, a["ws"], BIG, None)
    refused("cgic_spatial_norm_train", CAPACITY, "spatial_norm: workspace of 0 bytes, need 2304", *fwd, a["stats"], None, 0, None)
    fwd[10] = -1.0
    refused("cgic_spatial_norm_train", INVALID, "spatial_norm_train: eps -1", *fwd, a["stats"], a["ws"], BIG, None)
