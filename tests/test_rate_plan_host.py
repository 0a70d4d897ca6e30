"""The plans of the rate-control family (csrc/cgic_rate_plan.h) without a GPU: every check of cgic_rate_curve, cgic_rate_curve_tiles,
cgic_route_to_budget and cgic_rate_table in its order, the curve launch's threads, LDS bytes and staging, the grids of the launches
behind it, the layout of every workspace and the four size queries; and the router's rank arithmetic (cgic_encode_plan.h:
router_ranks), which the curve's coarse rank is a call of.  The headers are plain C++17: tests/host/rate_plan_main.cpp is compiled
with the host compiler alone -- once plainly, once with -fsanitize=address,undefined -- and run as a program over the table below,
whose rows were worked out by hand:
  the curve's LDS holds 12 bytes per 8x8 patch of the largest image / tile (n8 = 4 h16 w16), and behind them the 4 nsym bytes of
      code lengths when both fit 152 KB = 155648 bytes ("staged"); more than 64 KB needs the dynamic-LDS opt-in;
  threads: 1024, halved while >= n8 and above 256: 256 for n8 <= 512, 512 for 513 .. 1024, 1024 above;
  coarse rank: Python's round() of n16 * c, 0 (and mode 1) at c == 0;
  a workspace part is padded to 256 bytes: the summary is 16 bytes per image / tile; the budget route adds two blocks of 4 B R bytes;
      the tiles form adds 20 T M bytes (not padded) unless tile_nbytes is given; the rate table's three mask stacks hold C candidates
      of B n16, 4 B n16 and 16 B n16 int32, each candidate padded to 64 elements."""
import os
import shutil
import struct
import subprocess

import pytest

import specials_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2
CURVE, TILES, BUDGET, TABLE, Q_CURVE, Q_TILES, Q_BUDGET, Q_TABLE, RANKS = range(9)
WHO = {CURVE: "rate_curve", TILES: "rate_curve_tiles", BUDGET: "route_to_budget"}
ADDR = ("ind_c", "ind_m", "ind_f", "e16", "e8", "nbytes", "tiles_dev", "image_nbytes", "ranks_dev", "budget_dev", "mask_c", "mask_m",
        "mask_f", "ind", "choice_dev", "ws")
BASE = {k: (i + 1) << 36 for i, k in enumerate(ADDR)}           # 64 GiB apart, all 256-byte aligned


def bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def tile(h16, w16, k_c, shape=0, image=0, reserved=0, off=None):
    return dict(h16=h16, w16=w16, k_c=k_c, shape=shape, image=image, reserved=reserved, off=off)


def pack(tiles):
    """descriptors laid out one behind the other (an `off` of its own wins) -> (the five element counts, 33 numbers)"""
    at, nums = [0] * 5, []
    for t in tiles:
        n16 = t["h16"] * t["w16"]
        size = [n16, 4 * n16, 16 * n16, n16, 4 * n16]
        off = t["off"] or list(at)
        nums += [t["h16"], t["w16"], t["k_c"], t["shape"], t["image"], t["reserved"], *off]
        at = [a + s for a, s in zip(at, size)]
    return at, nums + [0] * (33 - len(nums))


def case(name, want, what, B=2, h16=4, w16=4, c=0.1, nsym=1024, max_len=24, table=1, R=0, T=0, N=1, S=1, M=1, given=0, C=0, inputs=1,
         tiles=(), count=None, count_given=1, tiles_given=1, ratio2=None, **addr):
    """addr: ws=+4 style byte offsets from the pointer's base, or None for NULL"""
    a = dict(BASE)
    for key, v in addr.items():
        a[key] = 0 if v is None else BASE[key] + v
    packed_count, desc = pack(tiles[:3])
    nums = [what, table, nsym, max_len, B, h16, w16, bits(c), bits(ratio2) if ratio2 is not None else R, T, N, S, M, given, C, inputs,
            *(a[k] for k in ADDR), count_given, *(count or packed_count), tiles_given, *desc]
    assert len(nums) == 72
    return pytest.param(" ".join(str(v) for v in nums), want, id=name)


def err(code, why):
    return dict(err=code, why=why)


def lds(n8, nsym):
    staged = sr.curve_staged(n8, nsym)
    return dict(staged=int(staged), lds=12 * n8 + (4 * nsym if staged else 0), opt_in=int(12 * n8 + (4 * nsym if staged else 0) > 65536))


LDS_MSG = "%s: %s of %d x %d coarse patches does not fit one workgroup's LDS (at most 12288 8x8 patches: 768x1024 pixels)"
WS_NULL = "%s: workspace of %d bytes required (cgic_%s_workspace_bytes)"
WS_ALIGN = "%s: the workspace must be 16-byte aligned"
ALIGN = "route_to_budget: ind_m, ind_f, mask_m, mask_f and ind must be 16-byte aligned, e8, the budget and the choice 8-byte aligned"
RATIO1 = "route_to_budget: coarse ratio %s outside [0, 1): the curve's mode is 0, or 1 at coarse ratio 0"
TWO = [tile(4, 4, 2, shape=0, image=0), tile(3, 5, 2, shape=1, image=1)]        # round(1.6) = 2, round(1.5) = 2
THREE = [tile(4, 4, 2), tile(4, 4, 2), tile(4, 4, 2)]

CASES = [
    # ---- LDS and staging (the issue's table)
    case("lds-4x4-16", dict(n8_max=64, staged=1, lds=832, opt_in=0, threads=256), CURVE, nsym=16),
    case("lds-48x64-1024", dict(n8_max=12288, staged=1, lds=151552, opt_in=1, threads=1024), CURVE, h16=48, w16=64, nsym=1024),
    case("lds-48x64-2048-equality", dict(staged=1, lds=155648, opt_in=1), CURVE, h16=48, w16=64, nsym=2048),
    case("lds-48x64-2049", dict(staged=0, lds=147456, opt_in=1), CURVE, h16=48, w16=64, nsym=2049),
    case("lds-4x4-38720-equality", dict(staged=1, lds=155648, opt_in=1), CURVE, nsym=38720),
    case("lds-4x4-38721", dict(staged=0, lds=768, opt_in=0), CURVE, nsym=38721),
    case("lds-4x4-65536", dict(staged=0, lds=768, opt_in=0), CURVE, nsym=65536),
    case("lds-budget-route-48x64", dict(staged=1, lds=151552, opt_in=1, threads=1024, grid=2), BUDGET, h16=48, w16=64, R=5),
    case("lds-tiles-by-the-largest", dict(n8_max=64, staged=1, lds=768 + 4096, opt_in=0, threads=256, grid=2), TILES, T=2, N=2, S=2, tiles=TWO),
    # ---- threads
    case("threads-8x16", dict(n8_max=512, threads=256), CURVE, h16=8, w16=16),
    case("threads-3x43", dict(n8_max=516, threads=512), CURVE, h16=3, w16=43),
    case("threads-16x16", dict(n8_max=1024, threads=512), CURVE, h16=16, w16=16),
    case("threads-16x17", dict(n8_max=1088, threads=1024), CURVE, h16=16, w16=17),
    case("threads-1x1", dict(n8_max=4, threads=256), CURVE, h16=1, w16=1),
    # ---- the coarse rank: halves to even
    case("rank-4-at-0.125", dict(k_c=0, mode=0), CURVE, h16=1, w16=4, c=0.125),
    case("rank-12-at-0.125", dict(k_c=2, mode=0), CURVE, h16=3, w16=4, c=0.125),
    case("rank-20-at-0.125", dict(k_c=2, mode=0), CURVE, h16=4, w16=5, c=0.125),
    case("rank-4x4-at-0.1", dict(k_c=2, mode=0), CURVE, c=0.1),
    case("rank-budget-4x4-at-0.1", dict(k_c=2, mode=0), BUDGET, c=0.1, R=1),
    case("rank-at-0", dict(k_c=0, mode=1), CURVE, c=0.0),
    case("rank-at-minus-0", dict(k_c=0, mode=1), CURVE, c=-0.0),
    case("rank-at-1-curve", dict(k_c=16, mode=0), CURVE, c=1.0),
    case("rank-at-1-tiles", dict(mode=0, grid=1), TILES, T=1, c=1.0, tiles=[tile(4, 4, 16)]),      # (a descriptor with k_c = n16 is the right one)
    case("rank-at-1-tiles-15", err(INVALID, "rate_curve_tiles: tile 0: k_coarse=15, the ratio gives 16 of 16"), TILES, T=1, c=1.0, tiles=[tile(4, 4, 15)]),
    case("rank-at-0-tiles", dict(mode=1, grid=1), TILES, T=1, c=0.0, tiles=[tile(4, 4, 0)]),
    case("rank-at-1-budget", err(INVALID, RATIO1 % "1"), BUDGET, c=1.0, R=1),
    case("ratio-nan", err(INVALID, "rate_curve: coarse ratio nan outside [0, 1]"), CURVE, c=float("nan")),
    case("ratio-above-1", err(INVALID, "rate_curve_tiles: coarse ratio 1.5 outside [0, 1]"), TILES, T=1, c=1.5, tiles=[tile(4, 4, 2)]),
    case("ratio-negative", err(INVALID, RATIO1 % "-0.1"), BUDGET, c=-0.1, R=1),
    # ---- limits
    case("limit-1x3073", err(UNSUPPORTED, LDS_MSG % ("rate_curve", "an image", 1, 3073)), CURVE, h16=1, w16=3073),
    case("limit-1x3072", dict(n8_max=12288), CURVE, h16=1, w16=3072),
    case("limit-64x64", err(UNSUPPORTED, LDS_MSG % ("route_to_budget", "an image", 64, 64)), BUDGET, h16=64, w16=64, R=1),
    case("limit-2^40-squared", err(UNSUPPORTED, LDS_MSG % ("rate_curve", "an image", 1 << 40, 1 << 40)), CURVE, h16=1 << 40, w16=1 << 40),
    case("limit-B-65536", err(UNSUPPORTED, "rate_curve: batch 65536 exceeds the grid limit"), CURVE, B=65536),
    case("limit-B-65535", dict(grid=65535, workspace=65535 * 16 + 16), CURVE, B=65535),
    case("B-0-curve", dict(nothing=1, grid=0, workspace=256), CURVE, B=0),
    case("B-0-budget", err(INVALID, "route_to_budget: bad shape"), BUDGET, B=0, R=1),
    case("B-negative", err(INVALID, "rate_curve: bad shape"), CURVE, B=-1),
    case("shape-0", err(INVALID, "rate_curve: an image: bad shape"), CURVE, h16=0),
    case("max-len-4095", dict(grid=2), CURVE, max_len=4095),
    case("max-len-4096", err(UNSUPPORTED, "rate_curve: codes of up to 4096 bits (at most 4095)"), CURVE, max_len=4096),
    case("nsym-65537", err(UNSUPPORTED, "route_to_budget: table of 65537 symbols"), BUDGET, nsym=65537, R=1),
    case("nsym-0", err(UNSUPPORTED, "rate_curve_tiles: table of 0 symbols"), TILES, T=1, nsym=0, tiles=[tile(4, 4, 2)]),
    # ---- workspaces
    case("ws-curve-B2", dict(nothing=0, workspace=256, off_summary=0, grid=2), CURVE),
    case("ws-budget-B2-R10", dict(workspace=768, off_summary=0, off_total=256, off_tkey=512, apply_grid=1, pick_grid=1, grid=2), BUDGET, R=10),
    case("ws-tiles-T3-M8", dict(workspace=736, off_summary=0, off_tile_nbytes=256, grid=3, fold_x=1, fold_y=1), TILES, T=3, M=8, tiles=THREE),
    case("ws-tiles-T3-M8-given", dict(workspace=256, grid=3), TILES, T=3, M=8, given=1, tiles=THREE),
    case("ws-tiles-T0-still-folds", dict(workspace=256 + 8 * 20, off_tile_nbytes=256, grid=0, fold_x=1, fold_y=2, nothing=0), TILES, T=0, N=2, M=8),
    case("ws-NULL", err(INVALID, WS_NULL % ("rate_curve", 256, "rate_curve")), CURVE, ws=None),
    case("ws-NULL-B0", err(INVALID, WS_NULL % ("rate_curve", 256, "rate_curve")), CURVE, B=0, ws=None),
    case("ws-NULL-budget", err(INVALID, WS_NULL % ("route_to_budget", 768, "route_to_budget")), BUDGET, R=10, ws=None),
    case("ws-NULL-tiles", err(INVALID, WS_NULL % ("rate_curve_tiles", 736, "rate_curve_tiles")), TILES, T=3, M=8, tiles=THREE, ws=None),
    case("ws+4", err(INVALID, WS_ALIGN % "rate_curve"), CURVE, ws=4),
    case("ws+4-tiles", err(INVALID, WS_ALIGN % "rate_curve_tiles"), TILES, T=3, M=8, tiles=THREE, ws=4),
    case("ws+16", dict(workspace=256), CURVE, ws=16),
    # ---- the budget route
    case("R-65", dict(workspace=256 + 2 * 768, off_tkey=256 + 768), BUDGET, R=65),
    case("R-66", err(INVALID, "route_to_budget: 66 requested ranks (1 .. 65)"), BUDGET, R=66),
    case("R-0", err(INVALID, "route_to_budget: 0 requested ranks (1 .. 65)"), BUDGET, R=0),
    case("apply-B64-16x16", dict(apply_grid=256, pick_grid=1, threads=512), BUDGET, B=64, h16=16, w16=16, R=1),
    case("apply-B65535-48x64", dict(apply_grid=65536, grid=65535), BUDGET, B=65535, h16=48, w16=64, R=1),
    case("align-e8+4", err(INVALID, ALIGN), BUDGET, R=1, e8=4),
    case("align-e8+8", dict(grid=2), BUDGET, R=1, e8=8),
    case("align-ind+8", err(INVALID, ALIGN), BUDGET, R=1, ind=8),
    case("align-mask_m+4", err(INVALID, ALIGN), BUDGET, R=1, mask_m=4),
    case("align-mask_c+4-is-free", dict(grid=2), BUDGET, R=1, mask_c=4),
    case("align-choice+4", err(INVALID, ALIGN), BUDGET, R=1, choice_dev=4),
    # ---- the tiles form
    case("fold-M300-N2", dict(fold_x=2, fold_y=2, grid=2), TILES, T=2, N=2, S=2, M=300, tiles=TWO),
    case("tiles-class-of-two-shapes", err(INVALID, "rate_curve_tiles: tile 1: shape class 0 holds tiles of two shapes"), TILES, T=2, N=2, S=2,
         tiles=[TWO[0], tile(3, 5, 2, shape=0, image=1)]),
    case("tiles-transposed-is-another-shape", err(INVALID, "rate_curve_tiles: tile 1: shape class 0 holds tiles of two shapes"), TILES, T=2,
         tiles=[tile(3, 5, 2), tile(5, 3, 2)]),
    case("tiles-k_c", err(INVALID, "rate_curve_tiles: tile 1: k_coarse=1, the ratio gives 2 of 15"), TILES, T=2, N=2, S=2,
         tiles=[TWO[0], tile(3, 5, 1, shape=1, image=1)]),
    case("tiles-part-past-its-buffer", err(INVALID, "rate_curve_tiles: tile 1: part 2 at offset 256 + 240 elements is outside its buffer of 495"),
         TILES, T=2, N=2, S=2, tiles=TWO, count=[31, 124, 495, 31, 124]),
    case("tiles-part-at-the-end", dict(grid=2), TILES, T=2, N=2, S=2, tiles=TWO, count=[31, 124, 496, 31, 124]),
    case("tiles-negative-offset", err(INVALID, "rate_curve_tiles: tile 0: part 0 at offset -1 + 16 elements is outside its buffer of 16"), TILES, T=1,
         tiles=[tile(4, 4, 2, off=[-1, 0, 0, 0, 0])]),
    case("tiles-reserved", err(INVALID, "rate_curve_tiles: tile 0: shape class 0 of 1, image 0 of 1"), TILES, T=1, tiles=[tile(4, 4, 2, reserved=7)]),
    case("tiles-shape-S", err(INVALID, "rate_curve_tiles: tile 1: shape class 2 of 2, image 1 of 2"), TILES, T=2, N=2, S=2,
         tiles=[TWO[0], tile(3, 5, 2, shape=2, image=1)]),
    case("tiles-image-N", err(INVALID, "rate_curve_tiles: tile 1: shape class 1 of 2, image 2 of 2"), TILES, T=2, N=2, S=2,
         tiles=[TWO[0], tile(3, 5, 2, shape=1, image=2)]),
    case("tiles-tile-shape-0", err(INVALID, "rate_curve_tiles: tile 1: bad shape"), TILES, T=2, tiles=[TWO[0], tile(0, 5, 0)]),
    case("tiles-tile-too-large", err(UNSUPPORTED, LDS_MSG % ("rate_curve_tiles", "tile 0", 64, 64)), TILES, T=1, tiles=[tile(64, 64, 410)]),
    case("tiles-descriptor-4-of-5-is-empty", err(INVALID, "rate_curve_tiles: tile 3: bad shape"), TILES, T=5, tiles=THREE),
    case("tiles-counts", err(INVALID, "rate_curve_tiles: bad counts (T=-1, N=1, S=1, M=1)"), TILES, T=-1),
    case("tiles-grid-T", err(UNSUPPORTED, "rate_curve_tiles: 65536 tiles of 1 images exceed the grid limit (65535)"), TILES, T=65536),
    case("tiles-grid-N", err(UNSUPPORTED, "rate_curve_tiles: 1 tiles of 65536 images exceed the grid limit (65535)"), TILES, T=1, N=65536, tiles=THREE),
    case("tiles-S-17", err(UNSUPPORTED, "rate_curve_tiles: 17 tile shapes (at most 16)"), TILES, T=1, S=17, tiles=THREE),
    case("tiles-S-16", dict(grid=1), TILES, T=1, S=16, tiles=THREE),
    case("tiles-M-65537", err(UNSUPPORTED, "rate_curve_tiles: 65537 settings (at most 65536)"), TILES, T=1, M=65537, tiles=THREE),
    case("tiles-negative-count", err(INVALID, "rate_curve_tiles: negative element count"), TILES, T=1, tiles=THREE, count=[16, 64, 256, -1, 64]),
    # ---- NULL arguments: each entry point's own list
    *[case(f"NULL-curve-{k}", err(INVALID, "rate_curve: NULL argument"), CURVE, **{k: None}) for k in ("ind_c", "ind_m", "ind_f", "e16", "e8", "nbytes")],
    case("NULL-curve-table", err(INVALID, "rate_curve: NULL argument"), CURVE, table=0, nsym=0),
    case("NULL-curve-others-do-not-matter", dict(grid=2), CURVE, tiles_dev=None, image_nbytes=None, ranks_dev=None, budget_dev=None, mask_c=None,
         mask_m=None, mask_f=None, ind=None, choice_dev=None, count_given=0, tiles_given=0),
    *[case(f"NULL-tiles-{k}", err(INVALID, "rate_curve_tiles: NULL argument"), TILES, T=1, tiles=THREE, **{k: None})
      for k in ("e8", "tiles_dev", "ranks_dev", "image_nbytes")],
    case("NULL-tiles-count", err(INVALID, "rate_curve_tiles: NULL argument"), TILES, T=1, tiles=THREE, count_given=0),
    case("NULL-tiles-descriptors", err(INVALID, "rate_curve_tiles: NULL argument"), TILES, T=1, tiles=THREE, tiles_given=0),
    *[case(f"NULL-budget-{k}", err(INVALID, "route_to_budget: NULL argument"), BUDGET, R=1, **{k: None})
      for k in ("ind_c", "ranks_dev", "budget_dev", "mask_c", "mask_m", "mask_f", "ind", "choice_dev")],
    case("NULL-budget-nbytes-does-not-matter", dict(grid=2), BUDGET, R=1, nbytes=None, tiles_dev=None, image_nbytes=None),
    # ---- which of two faults speaks (the first in the entry point's order)
    case("order-curve-NULL-before-ratio", err(INVALID, "rate_curve: NULL argument"), CURVE, c=2.0, e16=None),
    case("order-curve-ratio-before-table", err(INVALID, "rate_curve: coarse ratio 2 outside [0, 1]"), CURVE, c=2.0, nsym=0),
    case("order-curve-nsym-before-max-len", err(UNSUPPORTED, "rate_curve: table of 0 symbols"), CURVE, nsym=0, max_len=5000),
    case("order-curve-table-before-batch", err(UNSUPPORTED, "rate_curve: codes of up to 5000 bits (at most 4095)"), CURVE, max_len=5000, B=-1),
    case("order-curve-batch-before-shape", err(UNSUPPORTED, "rate_curve: batch 65536 exceeds the grid limit"), CURVE, B=65536, h16=0),
    case("order-curve-shape-before-workspace", err(UNSUPPORTED, LDS_MSG % ("rate_curve", "an image", 64, 64)), CURVE, h16=64, w16=64, ws=None),
    case("order-curve-workspace-before-empty-batch", err(INVALID, WS_ALIGN % "rate_curve"), CURVE, B=0, ws=4),
    case("order-tiles-NULL-before-counts", err(INVALID, "rate_curve_tiles: NULL argument"), TILES, T=1, M=0, tiles=THREE, ranks_dev=None),
    case("order-tiles-counts-before-ratio", err(INVALID, "rate_curve_tiles: bad counts (T=1, N=1, S=1, M=0)"), TILES, T=1, M=0, c=2.0, tiles=THREE),
    case("order-tiles-ratio-before-grid", err(INVALID, "rate_curve_tiles: coarse ratio 2 outside [0, 1]"), TILES, T=65536, c=2.0),
    case("order-tiles-table-before-grid", err(UNSUPPORTED, "rate_curve_tiles: table of 70000 symbols"), TILES, T=65536, nsym=70000),
    case("order-tiles-grid-before-shapes", err(UNSUPPORTED, "rate_curve_tiles: 65536 tiles of 1 images exceed the grid limit (65535)"), TILES, T=65536, S=17),
    case("order-tiles-shapes-before-settings", err(UNSUPPORTED, "rate_curve_tiles: 17 tile shapes (at most 16)"), TILES, T=1, S=17, M=65537, tiles=THREE),
    case("order-tiles-settings-before-counts", err(UNSUPPORTED, "rate_curve_tiles: 65537 settings (at most 65536)"), TILES, T=1, M=65537, tiles=THREE,
         count=[-1, 64, 256, 16, 64]),
    case("order-tiles-count-before-descriptor", err(INVALID, "rate_curve_tiles: negative element count"), TILES, T=1, tiles=[tile(0, 0, 0)],
         count=[-1, 64, 256, 16, 64]),
    case("order-tiles-first-descriptor-first", err(INVALID, "rate_curve_tiles: tile 0: k_coarse=3, the ratio gives 2 of 16"), TILES, T=2,
         tiles=[tile(4, 4, 3), tile(0, 0, 0)]),
    case("order-tiles-shape-before-class", err(INVALID, "rate_curve_tiles: tile 0: bad shape"), TILES, T=1, tiles=[tile(0, 4, 2, shape=5)]),
    case("order-tiles-class-before-two-shapes", err(INVALID, "rate_curve_tiles: tile 1: shape class 0 of 1, image 1 of 1"), TILES, T=2,
         tiles=[tile(4, 4, 2), tile(3, 5, 2, image=1)]),
    case("order-tiles-two-shapes-before-k_c", err(INVALID, "rate_curve_tiles: tile 1: shape class 0 holds tiles of two shapes"), TILES, T=2,
         tiles=[tile(4, 4, 2), tile(3, 5, 9)]),
    case("order-tiles-k_c-before-parts", err(INVALID, "rate_curve_tiles: tile 0: k_coarse=3, the ratio gives 2 of 16"), TILES, T=1,
         tiles=[tile(4, 4, 3)], count=[0, 0, 0, 0, 0]),
    case("order-tiles-descriptor-before-workspace", err(INVALID, "rate_curve_tiles: tile 0: k_coarse=3, the ratio gives 2 of 16"), TILES, T=1,
         tiles=[tile(4, 4, 3)], ws=None),
    case("order-budget-ratio-before-batch", err(INVALID, RATIO1 % "1"), BUDGET, c=1.0, B=0, R=1),
    case("order-budget-batch-before-ranks", err(INVALID, "route_to_budget: bad shape"), BUDGET, B=0, R=0),
    case("order-budget-shape-before-ranks", err(INVALID, "route_to_budget: an image: bad shape"), BUDGET, w16=0, R=0),
    case("order-budget-ranks-before-workspace", err(INVALID, "route_to_budget: 0 requested ranks (1 .. 65)"), BUDGET, R=0, ws=None),
    case("order-budget-workspace-before-alignment", err(INVALID, WS_NULL % ("route_to_budget", 768, "route_to_budget")), BUDGET, R=1, ws=None, e8=4),
    case("order-budget-workspace-alignment-before-the-others", err(INVALID, WS_ALIGN % "route_to_budget"), BUDGET, R=1, ws=8, e8=4),
    # ---- the size queries: the shape part alone
    case("query-curve-64", dict(bytes=1024), Q_CURVE, B=64, h16=16, w16=16),
    case("query-curve-2", dict(bytes=256), Q_CURVE),
    case("query-curve-B0", dict(bytes=0), Q_CURVE, B=0, h16=16, w16=16),
    case("query-curve-h0", dict(bytes=0), Q_CURVE, B=1, h16=0, w16=16),
    case("query-curve-w-negative", dict(bytes=0), Q_CURVE, B=1, h16=4, w16=-4),
    case("query-curve-beyond-the-grid", dict(bytes=0), Q_CURVE, B=65536),
    case("query-curve-beyond-the-LDS", dict(bytes=0), Q_CURVE, h16=64, w16=64),
    case("query-tiles-own", dict(bytes=256 + 6 * 1000 * 20), Q_TILES, T=6, M=1000),
    case("query-tiles-given", dict(bytes=256), Q_TILES, T=6, M=1000, given=1),
    case("query-tiles-T3-M8", dict(bytes=736), Q_TILES, T=3, M=8),
    case("query-tiles-T0", dict(bytes=0), Q_TILES, T=0, M=10, given=1),
    case("query-tiles-M0", dict(bytes=0), Q_TILES, T=6, M=0),
    case("query-tiles-M-65537", dict(bytes=0), Q_TILES, T=6, M=65537, given=1),
    case("query-tiles-T-65536", dict(bytes=0), Q_TILES, T=65536, M=1, given=1),
    case("query-tiles-T-65535", dict(bytes=65535 * 16 + 16), Q_TILES, T=65535, M=1, given=1),
    case("query-budget-64-923", dict(bytes=1024 + 2 * 64 * 923 * 4), Q_BUDGET, B=64, h16=16, w16=16, R=923),
    case("query-budget-R-1025", dict(bytes=256 + 2 * 4352), Q_BUDGET, B=1, h16=16, w16=16, R=1025),
    case("query-budget-2-10", dict(bytes=768), Q_BUDGET, R=10),
    *[case(f"query-budget-bad-{i}", dict(bytes=0), Q_BUDGET, B=b, h16=h, w16=w, R=r)
      for i, (b, h, w, r) in enumerate([(0, 16, 16, 4), (1, 0, 16, 4), (1, 16, -1, 4), (1, 16, 16, 0), (65536, 4, 4, 4), (1, 64, 64, 4),
                                         (1, 1, 3073, 4), (1, 16, 16, 1026), (1, 12289, 1, 4)])],
    case("query-table-64-16", dict(bytes=16 * 4 * (16384 + 65536 + 262144)), Q_TABLE, B=64, h16=16, w16=16, C=16),
    case("query-table-2-4x4-C3", dict(bytes=8448), Q_TABLE, C=3),
    case("query-table-C-65", dict(bytes=0), Q_TABLE, B=1, h16=1, w16=1, C=65),
    case("query-table-C-0", dict(bytes=0), Q_TABLE, C=0),
    case("query-table-B0", dict(bytes=0), Q_TABLE, B=0, h16=16, w16=16, C=4),
    case("query-table-h0", dict(bytes=0), Q_TABLE, h16=0, C=4),
    case("query-table-beyond-the-grid", dict(bytes=0), Q_TABLE, B=65536, C=4),
    # ---- the rate table
    case("table-2-4x4-C3", dict(nothing=0, stride_c=64, stride_m=128, stride_f=512, off_c=0, off_m=768, off_f=2304, workspace=8448, grid_x=2, grid_y=3,
                                lds=4096), TABLE, C=3),
    case("table-3x5-C1", dict(stride_c=64, stride_m=128, stride_f=512, off_m=256, off_f=768, workspace=2816), TABLE, h16=3, w16=5, C=1),
    case("table-lds-16384", dict(lds=65536), TABLE, C=1, nsym=16384),
    case("table-lds-16385", dict(lds=0), TABLE, C=1, nsym=16385),
    case("table-B0", dict(nothing=1, workspace=0), TABLE, B=0, C=1, nsym=0, ws=None),
    case("table-NULL-input", err(INVALID, "rate_table: NULL argument"), TABLE, C=3, inputs=0),
    case("table-NULL-table", err(INVALID, "rate_table: NULL argument"), TABLE, C=3, table=0, nsym=0),
    case("table-C-0", err(INVALID, "rate_table: 0 candidates (1..64)"), TABLE, C=0),
    case("table-C-65", err(INVALID, "rate_table: 65 candidates (1..64)"), TABLE, C=65),
    case("table-C-64", dict(grid_y=64, workspace=64 * 2816), TABLE, C=64),
    case("table-shape", err(INVALID, "rate_table: bad shape"), TABLE, C=1, w16=0),
    case("table-B-65536", err(UNSUPPORTED, "rate_table: batch 65536 exceeds the grid limit"), TABLE, C=1, B=65536),
    case("table-grid-2^26", err(UNSUPPORTED, "rate_table: latent grid too large"), TABLE, C=1, B=1, h16=2048, w16=2048),
    case("table-grid-2^40-squared", err(UNSUPPORTED, "rate_table: latent grid too large"), TABLE, C=1, B=1, h16=1 << 40, w16=1 << 40),
    case("table-nsym-65537", err(UNSUPPORTED, "rate_table: table of 65537 symbols"), TABLE, C=1, nsym=65537),
    case("table-bits-128", err(UNSUPPORTED, "rate_table: a stream could exceed 2^32 bits"), TABLE, C=1, B=1, h16=2048, w16=1024, max_len=128),
    case("table-bits-127", dict(stride_c=1 << 21, grid_x=1), TABLE, C=1, B=1, h16=2048, w16=1024, max_len=127),
    case("table-ws-NULL", err(INVALID, "rate_table: workspace of 8448 bytes required (cgic_rate_table_workspace_bytes)"), TABLE, C=3, ws=None),
    case("table-ws+4", err(INVALID, "rate_table: the workspace must be 16-byte aligned"), TABLE, C=3, ws=4),
    case("order-table-NULL-before-candidates", err(INVALID, "rate_table: NULL argument"), TABLE, C=0, inputs=0),
    case("order-table-candidates-before-shape", err(INVALID, "rate_table: 65 candidates (1..64)"), TABLE, C=65, h16=0),
    case("order-table-shape-before-batch", err(INVALID, "rate_table: bad shape"), TABLE, C=1, B=65536, h16=0),
    case("order-table-empty-batch-before-the-table", dict(nothing=1), TABLE, C=1, B=0, h16=1 << 20, w16=1 << 20, nsym=0, ws=None),
    case("order-table-grid-before-table", err(UNSUPPORTED, "rate_table: latent grid too large"), TABLE, C=1, B=1, h16=2048, w16=2048, nsym=0),
    case("order-table-table-before-bits", err(UNSUPPORTED, "rate_table: table of 0 symbols"), TABLE, C=1, B=1, h16=2048, w16=1024, max_len=128, nsym=0),
    case("order-table-bits-before-workspace", err(UNSUPPORTED, "rate_table: a stream could exceed 2^32 bits"), TABLE, C=1, B=1, h16=2048, w16=1024,
         max_len=128, ws=None),
    # ---- the rank arithmetic itself (B is n16): the router's modes, halves to even, and a k outside its list
    case("ranks-mode0", dict(ok=1, mode=0, k_c=26, k_m=922), RANKS, B=256, c=0.1, ratio2=0.8),          # round(25.6), round(102.4 + 819.2)
    case("ranks-mode0-halves", dict(ok=1, mode=0, k_c=2, k_m=12), RANKS, B=20, c=0.125, ratio2=0.03125),  # round(2.5), round(10 + 2.5)
    case("ranks-mode1", dict(ok=1, mode=1, k_c=0, k_m=410), RANKS, B=256, c=0.0, ratio2=0.4),           # round(409.6)
    case("ranks-mode2", dict(ok=1, mode=2, k_c=102, k_m=0), RANKS, B=256, c=0.4, ratio2=0.0),           # round(102.4)
    case("ranks-mode3", dict(ok=1, mode=3, k_c=77, k_m=0), RANKS, B=256, c=0.3, ratio2=0.7),            # round(76.8)
    case("ranks-mode4", dict(ok=1, mode=4, k_c=0, k_m=0), RANKS, B=256, c=1.0, ratio2=0.0),
    case("ranks-above-the-list", dict(ok=0, mode=0, k_c=384, k_m=1946), RANKS, B=256, c=1.5, ratio2=0.4),
    case("ranks-nan", dict(ok=0, mode=0), RANKS, B=256, c=float("nan"), ratio2=0.4),
]

# the staging rule of tests/specials_ref.py against the plan's: the issue's four shapes, and the boundary at the small end
# (768 + 4 * 38720 == 155648) with the two table sizes on either side of it and two further out
STAGED = [(64, 16), (12288, 1024), (12288, 2048), (12288, 2049), (64, 38720), (64, 38721), (64, 38896), (64, 38897)]
CASES += [case(f"staged-{n8}-{nsym}", lds(n8, nsym), CURVE, h16={64: 4, 12288: 48}[n8], w16={64: 4, 12288: 64}[n8], nsym=nsym) for n8, nsym in STAGED]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "rate_plan_main.cpp"), "-o", exe])
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
            parsed[c.id] = {k: v if v in ("nan", "-nan") else int(v) for k, v in (t.split("=", 1) for t in line.split())}
    return parsed


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("rate_plan"), [], "rate_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_rate_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_rate_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "rate_plan_main_san")
    assert _run(exe) == plans


def test_the_library_answers_as_the_plan_does(plans):
    """the four size queries of the loaded library are the plan's shape part: every query row of the table, asked of the library"""
    from control_gic_amd import _lib
    lib = _lib.lib()
    asked = 0
    for c in CASES:
        n = [int(v) for v in c.values[0].split()]
        what, B, h16, w16, R, T, M, given, C = n[0], n[4], n[5], n[6], n[8], n[9], n[12], n[13], n[14]
        want = plans[c.id].get("bytes")
        if what == Q_CURVE:
            assert lib.cgic_rate_curve_workspace_bytes(B, h16, w16) == want, c.id
        elif what == Q_TILES:
            assert lib.cgic_rate_curve_tiles_workspace_bytes(T, M, given) == want, c.id
        elif what == Q_BUDGET:
            assert lib.cgic_route_to_budget_workspace_bytes(B, h16, w16, R) == want, c.id
        elif what == Q_TABLE:
            assert lib.cgic_rate_table_workspace_bytes(B, h16, w16, C, 1) == want, c.id
        else:
            continue
        asked += 1
    assert asked >= 30
