"""The launch plan of the merge / pool / blend calls, _f32 and _h (csrc/cgic_merge_plan.h), without a GPU: the shape checks, the
accepted type pairs, the unit (consecutive x per thread), the aliasing rule and the grid.  The header is plain C++17:
tests/host/merge_plan_main.cpp is compiled with the host compiler alone -- once plainly, once with -fsanitize=address,undefined --
and run as a program over the table below, whose rows were worked out by hand:
  a thread that takes `unit` x reads max(1, unit / scale) elements of a tensor at 1 / scale of the grid in one access of at most
  16 bytes, and every pointer must be aligned to that access; unit = the largest of 8, 4, 2, 1 (fp32 features: of 4, 2, 1 -- 16
  bytes of the feature type) that divides the row width and that every pointer allows (the pool: input elements per row and
  thread, a multiple of k, for fp32 features k itself; 0 = element by element);
  total = B * C * h * (w / unit) (the pool: planes * (H / k) * (W / unit), unit 0 counting as k);
  grid = min(ceil(total / 256), 8192 for the merge, 16384 for the others)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2
F32, F16, BF16 = 0, 1, 2
MERGE, POOL, MEDIUM, FINE = 0, 1, 2, 3
ENTRY_H, ENTRY_F32 = 0, 1
BASE = {"f0": 0x10000000, "f1": 0x11000000, "f2": 0x12000000, "m0": 0x13000000, "m1": 0x14000000, "m2": 0x15000000, "out": 0x16000000}
ORDER = ("f0", "f1", "f2", "m0", "m1", "m2", "out")
OVERLAP = "out overlaps an input (only out == h with equal types, the blends' in-place form, may)"


def case(name, want, op, dt_in, dt_out, B, C, h, w, k=0, entry=ENTRY_H, **addr):
    """addr: f0=+8 style byte offsets from the tensor's 16 MiB-aligned base, or absolute addresses as ("abs", value)"""
    a = dict(BASE)
    for key, v in addr.items():
        a[key] = v[1] if isinstance(v, tuple) else BASE[key] + v
    line = " ".join(str(v) for v in (op, dt_in, dt_out, B, C, h, w, k, *(a[key] for key in ORDER), entry))
    return pytest.param(line, want, id=name)


def plan(unit, total, grid, in_place=0):
    return dict(unit=unit, total=total, grid=grid, in_place=in_place, threads=256)


def err(code, why):
    return dict(err=code, why=why)


CASES = []
# ---- the unit by row width (aligned pointers): fine blend and merge on [1,1,4,w], medium blend on [1,1,2,w]
for w, unit in ((4, 4), (8, 8), (12, 4), (16, 8), (20, 4)):
    CASES += [case(f"fine-w{w}", plan(unit, 4 * w // unit, 1), FINE, F16, F32, 1, 1, 4, w),
              case(f"merge-w{w}", plan(unit, 4 * w // unit, 1), MERGE, BF16, BF16, 1, 1, 4, w)]
for w, unit in ((2, 2), (6, 2), (10, 2), (4, 4), (8, 8), (12, 4)):
    CASES.append(case(f"medium-w{w}", plan(unit, 2 * w // unit, 1), MEDIUM, BF16, F32, 1, 1, 2, w))
# ---- the unit by pointer alignment: fine blend on [1,1,4,16] (64 elements)
CASES += [
    case("fine-h+2", plan(1, 64, 1), FINE, F16, F32, 1, 1, 4, 16, f0=2),
    case("fine-h+4", plan(2, 32, 1), FINE, F16, F32, 1, 1, 4, 16, f0=4),
    case("fine-h+8", plan(4, 16, 1), FINE, F16, F32, 1, 1, 4, 16, f0=8),
    case("fine-h+16", plan(8, 8, 1), FINE, F16, F32, 1, 1, 4, 16, f0=16),
    case("fine-own+8", plan(4, 16, 1), FINE, BF16, BF16, 1, 1, 4, 16, f1=8),
    # fp32 out: 4 * unit bytes per thread (two 16-byte stores at unit 8)
    case("fine-out32+4", plan(1, 64, 1), FINE, F16, F32, 1, 1, 4, 16, out=4),
    case("fine-out32+8", plan(2, 32, 1), FINE, F16, F32, 1, 1, 4, 16, out=8),
    case("fine-out32+16", plan(8, 8, 1), FINE, F16, F32, 1, 1, 4, 16, out=16),
    case("fine-out16+8", plan(4, 16, 1), FINE, F16, F16, 1, 1, 4, 16, out=8),
    case("fine-out16+2", plan(1, 64, 1), FINE, F16, F16, 1, 1, 4, 16, out=2),
    # masks: the fine one 4 * unit bytes, the medium one 2 * unit, the coarse one unit (4 at least)
    case("fine-mf+4", plan(1, 64, 1), FINE, F16, F32, 1, 1, 4, 16, m2=4),
    case("fine-mf+8", plan(2, 32, 1), FINE, F16, F32, 1, 1, 4, 16, m2=8),
    case("fine-mm+4", plan(2, 32, 1), FINE, F16, F32, 1, 1, 4, 16, m1=4),
    case("fine-mm+8", plan(4, 16, 1), FINE, F16, F32, 1, 1, 4, 16, m1=8),
    case("fine-mc+4", plan(4, 16, 1), FINE, F16, F32, 1, 1, 4, 16, m0=4),
    # the merge's coarser features: unit / 4 and unit / 2 halves per thread
    case("merge-hc+2", plan(4, 16, 1), MERGE, F16, F32, 1, 1, 4, 16, f0=2),
    case("merge-hc+4", plan(8, 8, 1), MERGE, F16, F32, 1, 1, 4, 16, f0=4),
    case("merge-hm+2", plan(2, 32, 1), MERGE, F16, F32, 1, 1, 4, 16, f1=2),
    case("merge-hm+4", plan(4, 16, 1), MERGE, F16, F32, 1, 1, 4, 16, f1=4),
    case("merge-hf+2", plan(1, 64, 1), MERGE, F16, F32, 1, 1, 4, 16, f2=2),
    case("medium-h+4-w6", plan(2, 6, 1), MEDIUM, F16, F32, 1, 1, 2, 6, f0=4),
    case("medium-h+2-w6", plan(1, 12, 1), MEDIUM, F16, F32, 1, 1, 2, 6, f0=2),
    # a pointer that is not aligned to its own element
    case("fine-h+1", err(INVALID, "decoder_blend_fine: a pointer is not aligned to its 2-byte element"), FINE, F16, F32, 1, 1, 4, 16, f0=1),
    case("fine-mf+2", err(INVALID, "decoder_blend_fine: a pointer is not aligned to its 4-byte element"), FINE, F16, F32, 1, 1, 4, 16, m2=2),
    case("merge-out32+2", err(INVALID, "grain_merge: a pointer is not aligned to its 4-byte element"), MERGE, BF16, F32, 1, 1, 4, 16, out=2),
    case("pool-x+1", err(INVALID, "avgpool: a pointer is not aligned to its 2-byte element"), POOL, BF16, BF16, 3, 1, 4, 8, 2, f0=1),
]
# ---- the pool on [3,4,W]: unit = input elements per row and thread, outputs per thread = unit / k
CASES += [
    case("pool2-w8", plan(8, 6, 1), POOL, F16, F16, 3, 1, 4, 8, 2),
    case("pool2-w4", plan(4, 6, 1), POOL, F16, F16, 3, 1, 4, 4, 2),
    case("pool2-w2", plan(2, 6, 1), POOL, F16, F16, 3, 1, 4, 2, 2),
    case("pool2-w12", plan(4, 18, 1), POOL, F16, F16, 3, 1, 4, 12, 2),
    case("pool2-w6", plan(2, 18, 1), POOL, F16, F16, 3, 1, 4, 6, 2),
    case("pool4-w8", plan(8, 3, 1), POOL, BF16, BF16, 3, 1, 4, 8, 4),
    case("pool4-w4", plan(4, 3, 1), POOL, BF16, BF16, 3, 1, 4, 4, 4),
    case("pool4-w12", plan(4, 9, 1), POOL, BF16, F32, 3, 1, 4, 12, 4),
    case("pool4-x+8", plan(4, 6, 1), POOL, BF16, BF16, 3, 1, 4, 8, 4, f0=8),
    case("pool4-x+4", plan(0, 6, 1), POOL, BF16, BF16, 3, 1, 4, 8, 4, f0=4),          # not even a window's row in one access
    case("pool2-x+4", plan(2, 24, 1), POOL, BF16, BF16, 3, 1, 4, 8, 2, f0=4),
    case("pool2-x+2", plan(0, 24, 1), POOL, BF16, BF16, 3, 1, 4, 8, 2, f0=2),
    case("pool2-out16+2", plan(2, 24, 1), POOL, F16, F16, 3, 1, 4, 8, 2, out=2),       # 4 outputs = 8 bytes, 2 = 4, 1 = 2
    case("pool2-out16+4", plan(4, 12, 1), POOL, F16, F16, 3, 1, 4, 8, 2, out=4),
    case("pool4-out32+4", plan(4, 6, 1), POOL, F16, F32, 3, 1, 4, 8, 4, out=4),        # 2 outputs = 8 bytes, 1 = 4
]
# ---- every type pair, for every call
NAMES = {MERGE: ("grain_merge", "cgic_grain_merge_f32"), POOL: ("avgpool", "cgic_avgpool_f32"),
         MEDIUM: ("decoder_blend_medium", "cgic_decoder_blend_medium_f32"), FINE: ("decoder_blend_fine", "cgic_decoder_blend_fine_f32")}
for op, (name, f32_call) in NAMES.items():
    shape = (3, 1, 8, 8, 2) if op == POOL else (1, 3, 8, 8, 0)
    total = 3 * 4 * 1 if op == POOL else 3 * 8 * 1
    for dt_in, dt_out in ((F16, F32), (F16, F16), (BF16, F32), (BF16, BF16)):
        CASES.append(case(f"{name}-types-{dt_in}{dt_out}", plan(8, total, 1), op, dt_in, dt_out, *shape))
    for dt_out in (F32, F16, BF16):
        CASES.append(case(f"{name}-types-0{dt_out}", err(UNSUPPORTED, f"{name}: fp32 features are {f32_call}'s; the _h call takes fp16 or bf16"),
                          op, F32, dt_out, *shape))
    CASES += [
        case(f"{name}-types-12", err(UNSUPPORTED, f"{name}: out_dtype 2 with in_dtype 1 (CGIC_DT_F32 or the features' own type)"), op, F16, BF16, *shape),
        case(f"{name}-types-21", err(UNSUPPORTED, f"{name}: out_dtype 1 with in_dtype 2 (CGIC_DT_F32 or the features' own type)"), op, BF16, F16, *shape),
        case(f"{name}-types-30", err(INVALID, f"{name}: in_dtype 3 (CGIC_DT_F16 or CGIC_DT_BF16)"), op, 3, F32, *shape),
        case(f"{name}-types-1-1", err(INVALID, f"{name}: out_dtype -1 with in_dtype 1 (CGIC_DT_F32 or the features' own type)"), op, F16, -1, *shape),
    ]
# ---- aliasing: [1,3,8,8] = 192 elements; out == h with equal types is the blends' in-place form, nothing else may overlap
H, OWN, MF = BASE["f0"], BASE["f1"], BASE["m2"]
for op, name in ((MEDIUM, "decoder_blend_medium"), (FINE, "decoder_blend_fine")):
    last_mask = BASE["m2"] if op == FINE else BASE["m1"]
    CASES += [
        case(f"{name}-in-place-f16", plan(8, 24, 1, 1), op, F16, F16, 1, 3, 8, 8, out=("abs", H)),
        case(f"{name}-in-place-bf16", plan(8, 24, 1, 1), op, BF16, BF16, 1, 3, 8, 8, out=("abs", H)),
        case(f"{name}-f32-out-on-h", err(INVALID, f"{name}: {OVERLAP}"), op, F16, F32, 1, 3, 8, 8, out=("abs", H)),
        case(f"{name}-out-on-own", err(INVALID, f"{name}: {OVERLAP}"), op, F16, F16, 1, 3, 8, 8, out=("abs", OWN)),
        case(f"{name}-out-inside-h", err(INVALID, f"{name}: {OVERLAP}"), op, F16, F16, 1, 3, 8, 8, out=("abs", H + 16)),
        case(f"{name}-out-ends-inside-h", err(INVALID, f"{name}: {OVERLAP}"), op, F16, F16, 1, 3, 8, 8, out=("abs", H - 368)),
        case(f"{name}-out-on-a-mask", err(INVALID, f"{name}: {OVERLAP}"), op, F16, F32, 1, 3, 8, 8, out=("abs", last_mask)),
        # 192 halves = 384 bytes: out ends where h begins, and begins where h ends
        case(f"{name}-out-before-h", plan(8, 24, 1), op, F16, F16, 1, 3, 8, 8, out=("abs", H - 384)),
        case(f"{name}-out-behind-h", plan(8, 24, 1), op, F16, F16, 1, 3, 8, 8, out=("abs", H + 384)),
        case(f"{name}-f32-out-ends-in-h", err(INVALID, f"{name}: {OVERLAP}"), op, F16, F32, 1, 3, 8, 8, out=("abs", H - 752)),
        case(f"{name}-f32-out-before-h", plan(8, 24, 1), op, F16, F32, 1, 3, 8, 8, out=("abs", H - 768)),
    ]
CASES += [
    case("merge-out-on-h_fine", err(INVALID, f"grain_merge: {OVERLAP}"), MERGE, F16, F16, 1, 3, 8, 8, out=("abs", BASE["f2"])),
    case("merge-out-on-h_coarse", err(INVALID, f"grain_merge: {OVERLAP}"), MERGE, F16, F16, 1, 3, 8, 8, out=("abs", BASE["f0"])),
    case("pool-out-on-x", err(INVALID, f"avgpool: {OVERLAP}"), POOL, F16, F16, 3, 1, 8, 8, 2, out=("abs", BASE["f0"])),
]
# ---- the grid caps: 8192 workgroups of 256 threads x 8 elements for the merge, 16384 for the others
CASES += [
    case("merge-below-cap", plan(8, 127 * 512 * 32, 8128), MERGE, BF16, F32, 1, 127, 512, 256),
    case("merge-at-cap", plan(8, 128 * 512 * 32, 8192), MERGE, BF16, F32, 1, 128, 512, 256),
    case("merge-past-cap", plan(8, 129 * 512 * 32, 8192), MERGE, BF16, F32, 1, 129, 512, 256),
    case("fine-at-cap", plan(8, 2 * 128 * 512 * 32, 16384), FINE, BF16, F32, 2, 128, 512, 256),
    case("fine-past-cap", plan(8, 2 * 130 * 512 * 32, 16384), FINE, BF16, F32, 2, 130, 512, 256),
    case("fine-one-block-past-cap", plan(8, 16385 * 256, 16384), FINE, BF16, F32, 1, 16385, 4, 512),
    case("medium-past-cap-unit2", plan(2, 2 * 130 * 128 * 255, 16384), MEDIUM, F16, F16, 2, 130, 128, 510),
    case("pool-past-cap", plan(8, 264 * 256 * 64, 16384), POOL, F16, F16, 264, 1, 512, 512, 2, out=("abs", 0x40000000)),
    case("fine-two-blocks", plan(4, 260, 2), FINE, F16, F32, 1, 65, 4, 4),
]
# ---- the shapes: the rules and the words of the _f32 entry points; the type pair is looked at first, an empty batch before NULL
NULLS = dict(f0=("abs", 0), f1=("abs", 0), f2=("abs", 0), m0=("abs", 0), m1=("abs", 0), m2=("abs", 0), out=("abs", 0))
CASES += [
    case("merge-6x8", err(INVALID, "grain_merge: fine grid 6x8 must be positive multiples of 4"), MERGE, F16, F32, 1, 1, 6, 8),
    case("fine-8x10", err(INVALID, "decoder_blend_fine: fine grid 8x10 must be positive multiples of 4"), FINE, F16, F32, 1, 1, 8, 10),
    case("fine-C0", err(INVALID, "decoder_blend_fine: fine grid 8x8 must be positive multiples of 4"), FINE, F16, F32, 1, 0, 8, 8),
    case("medium-3x4", err(INVALID, "decoder_blend_medium: medium grid 3x4 (need even height and width)"), MEDIUM, F16, F32, 1, 1, 3, 4),
    case("medium-4x3", err(INVALID, "decoder_blend_medium: medium grid 4x3 (need even height and width)"), MEDIUM, F16, F32, 1, 1, 4, 3),
    case("medium-B-1", err(INVALID, "decoder_blend_medium: medium grid 4x4 (need even height and width)"), MEDIUM, F16, F32, -1, 1, 4, 4),
    case("pool-k3", err(UNSUPPORTED, "avgpool: window 3; the decoder uses 4 and 2 (decoder.py:304-305)"), POOL, F16, F16, 1, 1, 9, 9, 3),
    case("pool-6x8-k4", err(INVALID, "avgpool: 6x8 is not a multiple of the window"), POOL, F16, F16, 1, 1, 6, 8, 4),
    case("pool-8x7-k2", err(INVALID, "avgpool: 8x7 is not a multiple of the window"), POOL, F16, F16, 1, 1, 8, 7, 2),
    case("fp32-before-the-shape", err(UNSUPPORTED, "grain_merge: fp32 features are cgic_grain_merge_f32's; the _h call takes fp16 or bf16"),
         MERGE, F32, F32, 1, 1, 6, 8),
    case("merge-empty-batch-NULL", plan(0, 0, 0), MERGE, F16, F32, 0, 3, 8, 8, **NULLS),
    case("pool-no-planes-NULL", plan(0, 0, 0), POOL, F16, F16, 0, 1, 8, 8, 2, **NULLS),
    case("merge-NULL", err(INVALID, "grain_merge: NULL tensor"), MERGE, F16, F32, 1, 3, 8, 8, **NULLS),
    case("fine-NULL-out", err(INVALID, "decoder_blend_fine: NULL tensor"), FINE, F16, F32, 1, 3, 8, 8, out=("abs", 0)),
    case("medium-NULL-mask", err(INVALID, "decoder_blend_medium: NULL tensor"), MEDIUM, F16, F32, 1, 3, 8, 8, m1=("abs", 0)),
    case("medium-unused-third-mask-NULL", plan(8, 24, 1), MEDIUM, F16, F32, 1, 3, 8, 8, m2=("abs", 0), f2=("abs", 0)),
    case("pool-NULL-x", err(INVALID, "avgpool: NULL tensor"), POOL, F16, F16, 1, 1, 8, 8, 2, f0=("abs", 0)),
]


# ---------------------------------------------------------------------------- fp32 features through the _f32 entry
def case32(name, want, op, B, C, h, w, k=0, **addr):
    return case(name, want, op, F32, F32, B, C, h, w, k, entry=ENTRY_F32, **addr)


# ---- unit 4 / 2 by row width: 16 bytes of fp32 are 4 elements, there is no unit 8
for w, unit in ((4, 4), (8, 4), (12, 4)):
    CASES += [case32(f"f32-fine-w{w}", plan(unit, 4 * w // unit, 1), FINE, 1, 1, 4, w),
              case32(f"f32-merge-w{w}", plan(unit, 4 * w // unit, 1), MERGE, 1, 1, 4, w)]
for w, unit in ((2, 2), (4, 4), (6, 2), (10, 2)):
    CASES.append(case32(f"f32-medium-w{w}", plan(unit, 2 * w // unit, 1), MEDIUM, 1, 1, 2, w))
# ---- the unit by pointer alignment on [1,1,4,16]: a feature or out on the grid 4 * unit bytes, the medium mask and the merge's
# medium feature 2 * unit (4 at least), the coarse ones 4
CASES += [
    case32("f32-fine-h+4", plan(1, 64, 1), FINE, 1, 1, 4, 16, f0=4),
    case32("f32-fine-h+8", plan(2, 32, 1), FINE, 1, 1, 4, 16, f0=8),
    case32("f32-fine-h+16", plan(4, 16, 1), FINE, 1, 1, 4, 16, f0=16),
    case32("f32-fine-out+4", plan(1, 64, 1), FINE, 1, 1, 4, 16, out=4),
    case32("f32-fine-out+8", plan(2, 32, 1), FINE, 1, 1, 4, 16, out=8),
    case32("f32-fine-out+16", plan(4, 16, 1), FINE, 1, 1, 4, 16, out=16),
    case32("f32-fine-mf+4", plan(1, 64, 1), FINE, 1, 1, 4, 16, m2=4),
    case32("f32-fine-mf+8", plan(2, 32, 1), FINE, 1, 1, 4, 16, m2=8),
    case32("f32-fine-mm+4", plan(2, 32, 1), FINE, 1, 1, 4, 16, m1=4),
    case32("f32-fine-mc+4", plan(4, 16, 1), FINE, 1, 1, 4, 16, m0=4),
    case32("f32-merge-hc+4", plan(4, 16, 1), MERGE, 1, 1, 4, 16, f0=4),
    case32("f32-merge-hm+4", plan(2, 32, 1), MERGE, 1, 1, 4, 16, f1=4),
    # a pointer that is not aligned to its own element: refused, where the kernels before the plan dereferenced it
    case32("f32-fine-h+2", err(INVALID, "decoder_blend_fine: a pointer is not aligned to its 4-byte element"), FINE, 1, 1, 4, 16, f0=2),
    case32("f32-merge-out+2", err(INVALID, "grain_merge: a pointer is not aligned to its 4-byte element"), MERGE, 1, 1, 4, 16, out=2),
    case32("f32-pool-x+2", err(INVALID, "avgpool: a pointer is not aligned to its 4-byte element"), POOL, 3, 1, 4, 8, 2, f0=2),
]
# ---- the pool on [3,4,W]: one output per thread; unit k = a window's row in one access, 0 = element by element
CASES += [
    case32("f32-pool4-w8", plan(4, 6, 1), POOL, 3, 1, 4, 8, 4),
    case32("f32-pool4-w4", plan(4, 3, 1), POOL, 3, 1, 4, 4, 4),
    case32("f32-pool4-x+8", plan(0, 6, 1), POOL, 3, 1, 4, 8, 4, f0=8),
    case32("f32-pool4-x+16", plan(4, 6, 1), POOL, 3, 1, 4, 8, 4, f0=16),
    case32("f32-pool2-w8", plan(2, 24, 1), POOL, 3, 1, 4, 8, 2),
    case32("f32-pool2-x+4", plan(0, 24, 1), POOL, 3, 1, 4, 8, 2, f0=4),
    case32("f32-pool2-x+8", plan(2, 24, 1), POOL, 3, 1, 4, 8, 2, f0=8),
    case32("f32-pool2-out+4", plan(2, 24, 1), POOL, 3, 1, 4, 8, 2, out=4),
    case32("f32-pool4-out+4", plan(4, 6, 1), POOL, 3, 1, 4, 8, 4, out=4),
]
# ---- aliasing, the half calls' rule: [1,3,8,8] = 192 floats = 768 bytes
for op, name in ((MEDIUM, "decoder_blend_medium"), (FINE, "decoder_blend_fine")):
    last_mask = BASE["m2"] if op == FINE else BASE["m1"]
    CASES += [
        case32(f"f32-{name}-in-place", plan(4, 48, 1, 1), op, 1, 3, 8, 8, out=("abs", H)),
        case32(f"f32-{name}-out-on-own", err(INVALID, f"{name}: {OVERLAP}"), op, 1, 3, 8, 8, out=("abs", OWN)),
        case32(f"f32-{name}-out-inside-h", err(INVALID, f"{name}: {OVERLAP}"), op, 1, 3, 8, 8, out=("abs", H + 16)),
        case32(f"f32-{name}-out-ends-inside-h", err(INVALID, f"{name}: {OVERLAP}"), op, 1, 3, 8, 8, out=("abs", H - 752)),
        case32(f"f32-{name}-out-on-a-mask", err(INVALID, f"{name}: {OVERLAP}"), op, 1, 3, 8, 8, out=("abs", last_mask)),
        case32(f"f32-{name}-out-before-h", plan(4, 48, 1), op, 1, 3, 8, 8, out=("abs", H - 768)),
        case32(f"f32-{name}-out-behind-h", plan(4, 48, 1), op, 1, 3, 8, 8, out=("abs", H + 768)),
    ]
CASES += [
    case32("f32-merge-out-on-h_fine", err(INVALID, f"grain_merge: {OVERLAP}"), MERGE, 1, 3, 8, 8, out=("abs", BASE["f2"])),
    case32("f32-pool-out-on-x", err(INVALID, f"avgpool: {OVERLAP}"), POOL, 3, 1, 8, 8, 2, out=("abs", BASE["f0"])),
]
# ---- the grid caps, in threads of 4 elements: B * C * h * (w / 4) against 8192 * 256 and 16384 * 256
CASES += [
    case32("f32-merge-at-cap", plan(4, 128 * 256 * 64, 8192), MERGE, 1, 128, 256, 256),
    case32("f32-merge-one-block-past-cap", plan(4, 8193 * 256, 8192), MERGE, 1, 8193, 4, 256),
    case32("f32-merge-one-row-past-cap", plan(4, 8192 * 256 + 4, 8192), MERGE, 1, 8192 * 64 + 1, 4, 4, f2=("abs", 0x100000000), out=("abs", 0x200000000)),
    case32("f32-fine-at-cap", plan(4, 16384 * 256, 16384), FINE, 1, 16384, 4, 256),
    case32("f32-fine-one-block-past-cap", plan(4, 16385 * 256, 16384), FINE, 1, 16385, 4, 256),
    case32("f32-medium-past-cap-unit2", plan(2, 2 * 130 * 128 * 255, 16384), MEDIUM, 2, 130, 128, 510, f1=("abs", 0x100000000), out=("abs", 0x200000000)),
    case32("f32-pool-past-cap", plan(2, 264 * 128 * 128, 16384), POOL, 264, 1, 256, 256, 2, out=("abs", 0x40000000)),
]
# ---- the shapes and the order of the checks, in the words the _f32 calls have always used; the types the _f32 entry fills in
CASES += [
    case32("f32-merge-6x8", err(INVALID, "grain_merge: fine grid 6x8 must be positive multiples of 4"), MERGE, 1, 1, 6, 8),
    case32("f32-fine-8x10", err(INVALID, "decoder_blend_fine: fine grid 8x10 must be positive multiples of 4"), FINE, 1, 1, 8, 10),
    case32("f32-medium-3x4", err(INVALID, "decoder_blend_medium: medium grid 3x4 (need even height and width)"), MEDIUM, 1, 1, 3, 4),
    case32("f32-pool-k3", err(UNSUPPORTED, "avgpool: window 3; the decoder uses 4 and 2 (decoder.py:304-305)"), POOL, 1, 1, 9, 9, 3),
    case32("f32-pool-8x7-k2", err(INVALID, "avgpool: 8x7 is not a multiple of the window"), POOL, 1, 1, 8, 7, 2),
    case32("f32-merge-empty-batch-NULL", plan(0, 0, 0), MERGE, 0, 3, 8, 8, **NULLS),
    case32("f32-pool-no-planes-NULL", plan(0, 0, 0), POOL, 0, 1, 8, 8, 2, **NULLS),
    case32("f32-shape-before-NULL", err(INVALID, "grain_merge: fine grid 6x8 must be positive multiples of 4"), MERGE, 1, 1, 6, 8, **NULLS),
    case32("f32-merge-NULL", err(INVALID, "grain_merge: NULL tensor"), MERGE, 1, 3, 8, 8, **NULLS),
    case32("f32-medium-NULL-mask", err(INVALID, "decoder_blend_medium: NULL tensor"), MEDIUM, 1, 3, 8, 8, m0=("abs", 0)),
    case32("f32-pool-NULL-out", err(INVALID, "avgpool: NULL tensor"), POOL, 1, 1, 8, 8, 2, out=("abs", 0)),
    case("f32-entry-with-halves", err(INVALID, "grain_merge: in_dtype 1 (CGIC_DT_F32)"), MERGE, F16, F32, 1, 3, 8, 8, entry=ENTRY_F32),
    case("f32-entry-half-out", err(UNSUPPORTED, "avgpool: out_dtype 2 with in_dtype 0 (CGIC_DT_F32 or the features' own type)"), POOL, F32, BF16,
         3, 1, 8, 8, 2, entry=ENTRY_F32),
]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "merge_plan_main.cpp"), "-o", exe])
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
    return _run(_build(tmp_path_factory.mktemp("merge_plan"), [], "merge_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_merge_half_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_merge_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "merge_plan_main_san")
    assert _run(exe) == plans
