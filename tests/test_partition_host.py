"""CPU: the partition map (cgic_partition_map, ABI 14) -- the shape of the ABI, every refusal of the entry point (dummy pointers: nothing
is launched), the CPU expectations of the GPU tests against each other and against the fixture of the REAL draw_triple_grain_256res
(tests/golden/partition.npz), grain_map, the custom op's fake-tensor shapes and the signatures that must not move."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, draw, highres
from conftest import ROOT
import partition_ref as ref

INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
SRC, OUT, OUT8, MC, MM, MF, IDX = 0x100000, 0x200000, 0x300000, 0x400000, 0x410000, 0x420000, 0x430000     # dummy addresses: never dereferenced


def test_abi_prototype_and_exports():
    assert _lib.lib().cgic_abi_version() >= 14
    assert len(_lib.PROTOTYPES["cgic_partition_map"][1]) == 10
    assert ctypes.sizeof(_lib.PartitionTile) == 64
    hdr = open(os.path.join(ROOT, "include", "cgic_hip.h")).read()
    assert int(re.search(r"^#define\s+CGIC_ABI_VERSION\s+(\d+)", hdr, re.M).group(1)) >= 14
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cgic_[a-z0-9_]+)\s*\(", code))
    assert "cgic_partition_map" in declared and declared == set(_lib.PROTOTYPES)
    assert hasattr(ctypes.CDLL(cg.LIB_PATH), "cgic_partition_map")
    # the struct as the header spells it: four pointers, the stride, six ints
    body = re.search(r"typedef struct cgic_partition_tile \{(.*?)\} cgic_partition_tile;", code, re.S).group(1)
    names = re.findall(r"\*?\b([a-z_0-9]+)\s*[,;]", body)
    assert names == [f[0] for f in _lib.PartitionTile._fields_]


def _tile(masks=True, y0=0, x0=0, th=16, tw=16, gh=0, gw=0, stride=1, mc=MC, mm=MM, mf=MF, idx=None):
    if not masks:
        mc = mm = mf = None
        idx = IDX if idx is None else idx
    return _lib.PartitionTile(mc, mm, mf, idx, stride, y0, x0, th, tw, gh, gw)


def _call(tiles, N=1, H=32, W=32, src=SRC, u8=0, f32=OUT, o8=None, n=None):
    arr = (_lib.PartitionTile * max(len(tiles), 1))(*tiles)
    return _lib.lib().cgic_partition_map(src, u8, N, H, W, len(tiles) if n is None else n, arr, f32, o8, None)


def test_every_refusal_comes_before_any_launch():
    # (N = 0 with valid arguments: every check passes and nothing is launched -- the only successful call a host test can make)
    assert _call([_tile()], N=0) == 0
    assert _call([_tile(), _tile(x0=16)], N=0, f32=None, o8=OUT8 + 1) == 0               # uint8 output: any address
    assert _call([_tile(masks=False, gh=4, gw=4)], N=0, u8=1, src=SRC + 1, f32=OUT, o8=OUT8) == 0
    assert _call([_tile(gh=4, gw=4)], N=0) == 0                                           # the masks' own grid may be named
    assert _call([_tile(masks=False, th=27, tw=41, gh=6, gw=10)], N=0, H=27, W=41) == 0  # ragged: any extent in indices form
    # NULLs and no output
    assert _lib.lib().cgic_partition_map(SRC, 0, 1, 32, 32, 1, None, OUT, None, None) == INVALID
    assert _call([_tile()], src=None) == INVALID
    assert _call([_tile()], f32=None, o8=None) == INVALID
    assert b"no output" in _lib.lib().cgic_last_error()
    # both forms in one tile, neither, a partial set of masks, mixed forms in one call
    assert _call([_tile(idx=IDX)]) == INVALID
    assert _call([_tile(mc=None, mm=None, mf=None)]) == INVALID
    assert _call([_tile(mf=None)]) == INVALID
    assert _call([_tile(mc=None, mm=None)]) == INVALID
    assert _call([_tile(), _tile(masks=False, x0=16, gh=4, gw=4)]) == INVALID
    assert b"same form" in _lib.lib().cgic_last_error()
    # shapes: masks form needs multiples of 16 and its own grid; indices form a cell of at least one pixel
    assert _call([_tile(th=24)]) == INVALID
    assert _call([_tile(tw=20)]) == INVALID
    assert _call([_tile(gh=2, gw=2)]) == INVALID
    assert _call([_tile(masks=False, gh=17, gw=4)]) == UNSUPPORTED                         # gh > th
    assert _call([_tile(masks=False, gh=4, gw=17)]) == UNSUPPORTED
    assert _call([_tile(masks=False, gh=0, gw=4)]) == INVALID
    assert _call([_tile(th=0)]) == INVALID
    assert _call([_tile(masks=False, th=70000, gh=4, gw=4)]) == UNSUPPORTED
    assert _call([_tile()], H=0) == INVALID
    assert _call([_tile()], W=70000) == UNSUPPORTED
    assert _call([_tile()], N=-1) == INVALID
    assert _call([_tile()], N=65536) == UNSUPPORTED
    assert _call([_tile(y0=1 << 30)]) == INVALID
    assert _call([_tile(stride=-1)]) == INVALID
    assert _call([_tile()], u8=2) == INVALID
    # alignment: fp32 images 4 bytes (the 16-byte path is chosen per address in the kernel), int32 masks 4, int64 indices 8
    assert _call([_tile()], src=SRC + 2) == INVALID
    assert _call([_tile()], f32=OUT + 2) == INVALID
    assert _call([_tile()], src=SRC + 4, f32=OUT + 4, N=0) == 0
    assert _call([_tile(mm=MM + 2)]) == INVALID
    assert _call([_tile(masks=False, gh=4, gw=4, idx=IDX + 4)]) == INVALID
    # overlap: of the CLIPPED tiles (two tiles that only share pad pixels do not overlap)
    assert _call([_tile(), _tile(y0=8, x0=8)]) == UNSUPPORTED
    assert b"overlap" in _lib.lib().cgic_last_error()
    assert _call([_tile(), _tile()]) == UNSUPPORTED
    assert _call([_tile(y0=-16, x0=-8), _tile(y0=-16, x0=0)], N=0) == 0
    assert _call([_tile(y0=-8, x0=-8), _tile(y0=-8, x0=0)]) == UNSUPPORTED
    # an output that overlaps the source without being it; the two outputs on each other
    nbytes = 3 * 32 * 32 * 4
    assert _call([_tile()], f32=SRC + 16) == INVALID                                       # a partial alias
    assert b"overlaps src" in _lib.lib().cgic_last_error()
    assert _call([_tile()], f32=SRC - nbytes + 4) == INVALID
    # (the ACCEPTING side of the alias rule cannot be shown here: a call that passes launches, so it needs N = 0, and with N = 0 every
    # range is empty.  The three N = 0 calls below only show that such addresses are not refused for another reason; that an exact
    # alias of the same layout is accepted and drawn right is tests/test_partition_map.py's in-place cases, on the device)
    assert _call([_tile()], f32=SRC - nbytes, N=0) == 0
    assert _call([_tile()], f32=None, o8=SRC) == INVALID                                   # the same address in ANOTHER layout
    assert _call([_tile()], u8=1, f32=SRC) == INVALID
    assert _call([_tile()], u8=1, f32=None, o8=SRC + 3) == INVALID
    assert _call([_tile()], f32=OUT, o8=OUT + 64) == INVALID
    assert _call([_tile()], f32=SRC, N=0) == 0 and _call([_tile()], u8=1, f32=None, o8=SRC, N=0) == 0
    # tile count: what a 4 KB argument block takes
    assert draw.MAX_TILES == 84
    assert _call([], n=0) == UNSUPPORTED
    assert _call([_tile(x0=16 * k) for k in range(85)], W=16 * 85) == UNSUPPORTED
    assert _call([_tile(x0=16 * k) for k in range(84)], W=16 * 84, N=0) == 0


def test_refused_inside_a_launch_group():
    l = _lib.lib()
    assert l.cgic_group_begin(2, None) == 0
    try:
        assert _call([_tile()], N=0) == INVALID
        assert b"cgic_partition_map" in l.cgic_last_error()
    finally:
        l.cgic_group_abort()


# ---- the expectations of the GPU tests: closed form == loop restatement == the real function's pictures ---------------------------
def test_closed_form_equals_the_loops_on_small_shapes():
    rng = np.random.default_rng(0)
    cases = [(1, 16, 16, 4, 4), (2, 32, 48, 8, 12), (1, 27, 41, 6, 10), (2, 5, 7, 5, 7), (1, 32, 48, 1, 8), (1, 19, 23, 3, 5), (1, 40, 24, 10, 3)]
    for B, H, W, gh, gw in cases:
        x = rng.random((B, 3, H, W)).astype(np.float32)
        for _ in range(3):
            ind = rng.integers(-1, 4, (B, gh, gw))
            assert np.array_equal(ref.closed_form(x, ind), ref.loop_draw(x, ind)), (B, H, W, gh, gw)


def test_expectations_equal_the_fixture_of_the_real_function(golden):
    g = golden("partition")
    keys = [(f"s{si}_r{ri}", f"s{si}_x") for si in range(3) for ri in range(7)] + [("malformed", "s1_x"), ("ragged", "ragged_x")]
    for key, xkey in keys:
        frames = g[xkey]
        x = ref.to_unit(frames)
        want = ref.decode_pic(g[f"{key}_pic"])
        if key[0] == "s":
            mc, mm, mf = (g[f"{key}_{m}"].astype(np.int32) for m in ("mc", "mm", "mf"))
            ind = ref.first_maximum(mc, mm, mf)
            assert np.array_equal(ind, g[f"{key}_ind"])
        else:
            ind = g[f"{key}_ind"]
        loop, closed = ref.loop_draw(x, ind), ref.closed_form(x, ind)
        assert np.array_equal(loop, want) and np.array_equal(closed, want), key
        line = np.stack([ref.line_mask(x.shape[2], x.shape[3], ind[b]) for b in range(x.shape[0])])
        assert np.array_equal(ref.to_frames(want, line), g[f"{key}_frames"]), key
        assert np.array_equal(ref.loop_draw(frames.transpose(0, 3, 1, 2).astype(np.int16), ind).transpose(0, 2, 3, 1) == -1,
                              np.repeat(line[..., None], 3, -1))
    assert g["malformed_ind"].shape == (2, 1, 8) and g["malformed_ind"].max() > 2
    for name in ("t0", "t1"):
        H, W, tile = (int(v) for v in g[f"{name}_hw_tile"])
        pad, tiles, _ = ref.geometry(H, W, tile)
        assert list(pad) == list(g[f"{name}_pad"]) and len(tiles) == int(g[f"{name}_ntiles"])
        inds = []
        for i, t in enumerate(tiles):
            assert list(t) == list(g[f"{name}_tile{i}"])                     # the real grid functions give this package's grid
            inds.append(ref.first_maximum(*(g[f"{name}_tile{i}_{m}"].astype(np.int32) for m in ("mc", "mm", "mf"))))
        x = ref.to_unit(g[f"{name}_x"])
        for drawer in (ref.loop_draw, ref.closed_form):
            pic, line = ref.tiled_expected(x, inds, pad, tiles, drawer)
            assert np.array_equal(pic, ref.decode_pic(g[f"{name}_pic"])) and np.array_equal(ref.to_frames(pic, line), g[f"{name}_frames"])


def test_byte_conversions_are_what_the_header_says():
    b = np.arange(256, dtype=np.uint8)
    unit = b.astype(np.float32) / np.float32(255)
    assert np.array_equal((np.float32(255.0) * unit).astype(np.uint8), b)         # uint8 -> fp32 -> uint8 is the identity
    pic = np.array([np.nan, np.inf, -np.inf, -0.0, 1.5, -0.25, 0.5, 254.999 / 255], dtype=np.float32).reshape(1, 1, 1, 8).repeat(3, 1)
    assert ref.to_frames(pic, np.zeros((1, 1, 8), bool))[0, 0, :, 0].tolist() == [0, 255, 0, 0, 255, 0, 127, 254]


def test_grain_map_on_partitions_and_on_masks_that_are_none():
    rng = np.random.default_rng(1)
    for B, H, W in ((1, 16, 16), (2, 32, 48), (3, 64, 32)):
        mc, mm, mf = ref.random_partition(rng, B, H, W)
        got = cg.grain_map([torch.from_numpy(m) for m in (mc, mm, mf)])
        assert got.dtype == torch.int64 and tuple(got.shape) == (B, H // 4, W // 4)
        assert np.array_equal(got.numpy(), ref.first_maximum(mc, mm, mf))
        assert np.array_equal((got.numpy() == 2), mf[:, 0] == 1)
        # not partitions: all zero, overlapping, values other than 0 / 1
        zero = [np.zeros_like(m) for m in (mc, mm, mf)]
        assert int(cg.grain_map([torch.from_numpy(m) for m in zero]).abs().max()) == 0
        ones = [np.ones_like(m) for m in (mc, mm, mf)]
        assert int(cg.grain_map([torch.from_numpy(m) for m in ones]).abs().max()) == 0          # coarse wins
        wild = [rng.integers(-2, 3, m.shape).astype(np.int32) * 7 for m in (mc, mm, mf)]
        assert np.array_equal(cg.grain_map([torch.from_numpy(m) for m in wild]).numpy(), ref.first_maximum(*wild))
        # without the singleton axis
        assert np.array_equal(cg.grain_map([torch.from_numpy(m[:, 0]) for m in (mc, mm, mf)]).numpy(), ref.first_maximum(mc, mm, mf))
    with pytest.raises(ValueError):
        cg.grain_map([torch.zeros(1, 1, 1, 1, dtype=torch.int32), torch.zeros(1, 1, 2, 2, dtype=torch.int32), torch.zeros(1, 1, 4, 5, dtype=torch.int32)])


def test_cpu_tensors_raise_and_arguments_are_checked():
    x = torch.zeros(1, 3, 16, 16)
    mask = [torch.zeros(1, 1, 1, 1, dtype=torch.int32), torch.zeros(1, 1, 2, 2, dtype=torch.int32), torch.zeros(1, 1, 4, 4, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match="HIP"):
        cg.partition_map(x, mask)
    with pytest.raises(RuntimeError, match="HIP"):
        cg.draw_triple_grain_256res(x, torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP"):
        cg.partition_tiles(x, [mask], tile=16)
    with pytest.raises(TypeError):
        cg.draw_triple_grain_256res(None, torch.zeros(1, 4, 4, dtype=torch.int64))


def test_partition_map_op_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        m = [torch.empty(2, 1, 2, 3, dtype=torch.int32, device="cuda"), torch.empty(2, 1, 4, 6, dtype=torch.int32, device="cuda"),
             torch.empty(2, 1, 8, 12, dtype=torch.int32, device="cuda")]
        x = torch.empty(2, 3, 32, 48, device="cuda")
        x8 = torch.empty(2, 32, 48, 3, dtype=torch.uint8, device="cuda")
        for src in (x, x8):
            out = torch.ops.cgic.partition_map(src, m[0], m[1], m[2], False)
            assert tuple(out.shape) == (2, 3, 32, 48) and out.dtype == torch.float32 and out.device.type == "cuda"
            fr = torch.ops.cgic.partition_map(src, m[0], m[1], m[2], True)
            assert tuple(fr.shape) == (2, 32, 48, 3) and fr.dtype == torch.uint8


def test_signatures_that_must_not_move():
    from control_gic_amd import model
    p = inspect.signature(model.compress).parameters
    assert list(p) == ["self", "input", "path", "h_indices", "h_mask", "save_img"]
    assert p["h_indices"].default is None and p["h_mask"].default is None and p["save_img"].default is False
    p = inspect.signature(model.compress_batch).parameters
    assert list(p)[:4] == ["model", "input", "h_indices", "decode"] and p["decode"].default is True and p["save_img"].default is False
    p = inspect.signature(cg.draw_triple_grain_256res).parameters
    assert list(p) == ["images", "indices"] and p["images"].default is None and p["indices"].default is None
    p = inspect.signature(cg.partition_map).parameters
    assert list(p) == ["x", "mask", "frames", "out"] and p["frames"].default is False and p["out"].default is None
    p = inspect.signature(highres.partition_tiles).parameters
    assert list(p)[:5] == ["x", "tiled", "frames", "out", "tile"] and p["tile"].default == highres.TILE
    assert hasattr(highres.TiledCall, "partition") and cg.partition_tiles is highres.partition_tiles
    assert cg.CompressedBatch.partition_map is None
    for name in ("partition_map", "partition_tiles", "grain_map", "draw_triple_grain_256res", "draw"):
        assert name in cg.__all__
