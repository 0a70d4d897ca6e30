"""CPU: the way out of the tiling driver (cgic_paste_tiles / cgic_tile_weights_host, ABI 13) -- the blend factors against the reference's,
every argument check of the two entry points (dummy pointers: nothing is launched), the grid check of paste_tiles and the custom op's
fake-tensor shapes."""
import ctypes

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, highres

INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
SRC, OUT, WX, WY = 0x10000, 0x20000, 0x30000, 0x40000              # dummy, suitably aligned "device" addresses: never dereferenced


def test_abi_and_prototypes():
    assert _lib.lib().cgic_abi_version() >= 13
    assert len(_lib.PROTOTYPES["cgic_paste_tiles"][1]) == 8 and len(_lib.PROTOTYPES["cgic_tile_weights_host"][1]) == 3
    assert ctypes.sizeof(_lib.PasteTile) == 48


@pytest.mark.parametrize("n", [16, 32, 48, 592, 768])
def test_factors_equal_gaussian_weights_bit_for_bit(n):
    for th, tw in ((n, n), (n, 16), (16, n)):
        got = torch.outer(highres.tile_weight_factors(th, 1), highres.tile_weight_factors(tw, 0))
        want = highres.gaussian_weights(tw, th)
        assert got.dtype == torch.float64 and torch.equal(got, want[0, 0])
        assert float(got.min().float()) > 1.2e-38                       # con = (float)w is neither zero nor subnormal


def test_factors_equal_the_references_weights(golden):
    g = golden("paste")
    for tw, th in ((16, 16), (32, 16), (48, 32), (16, 768)):
        got = torch.outer(highres.tile_weight_factors(th, 1), highres.tile_weight_factors(tw, 0)).numpy()
        want = g[f"weights_{tw}x{th}"]
        assert want.dtype == np.float64 and want.shape == (th, tw)
        assert np.array_equal(got, want)
        assert np.array_equal(highres.gaussian_weights(tw, th)[0, 0].numpy(), want)


def test_factors_are_cached_and_asymmetric():
    a = highres.tile_weight_factors(32, 0)
    assert highres.tile_weight_factors(32, 0) is a and a.device.type == "cpu"
    y = highres.tile_weight_factors(32, 1)
    assert torch.equal(a, a.flip(0)) and not torch.equal(y, y.flip(0))           # x: midpoint 15.5; y: midpoint 16 (the reference's)
    assert float(y[16]) == float(y.max())


def test_tile_weights_host_argument_checks():
    l = _lib.lib()
    buf = (ctypes.c_double * 4)()
    assert l.cgic_tile_weights_host(4, 0, buf) == 0
    assert l.cgic_tile_weights_host(0, 0, buf) == INVALID
    assert l.cgic_tile_weights_host(-3, 1, buf) == INVALID
    assert l.cgic_tile_weights_host(4, 2, buf) == INVALID
    assert l.cgic_tile_weights_host(4, -1, buf) == INVALID
    assert l.cgic_tile_weights_host(4, 0, None) == INVALID
    assert b"tile_weights_host" in l.cgic_last_error()
    with pytest.raises(cg.CgicError):
        highres.tile_weight_factors(0, 0)


def _tile(src=SRC, stride=3 * 16 * 16, wx=WX, wy=WY, y0=0, x0=0, th=16, tw=16):
    return _lib.PasteTile(src, stride, wx, wy, y0, x0, th, tw)


def _paste(tiles, N=1, H=32, W=32, f32=OUT, u8=None, n=None):
    arr = (_lib.PasteTile * max(len(tiles), 1))(*tiles)
    return _lib.lib().cgic_paste_tiles(N, H, W, len(tiles) if n is None else n, arr, f32, u8, None)


def test_paste_tiles_argument_checks_come_before_any_launch():
    # (N = 0 with valid arguments: every check passes and nothing is launched -- the only successful call a host test can make)
    assert _paste([_tile()], N=0) == 0
    assert _paste([_tile(), _tile(x0=16)], N=0, f32=None, u8=OUT + 1) == 0          # uint8 output: any address
    assert _paste([_tile(wx=None, wy=None)], N=0) == 0
    # NULLs
    assert _lib.lib().cgic_paste_tiles(1, 32, 32, 1, None, OUT, None, None) == INVALID
    assert _paste([_tile()], f32=None, u8=None) == INVALID                            # both outputs NULL
    assert _paste([_tile(src=None)]) == INVALID
    # alignment
    assert _paste([_tile(src=SRC + 4)]) == INVALID
    assert _paste([_tile(src=SRC + 8)]) == INVALID
    assert _paste([_tile(stride=3 * 16 * 16 + 2)]) == INVALID
    assert _paste([_tile(stride=-4)]) == INVALID
    assert _paste([_tile()], f32=OUT + 2) == INVALID
    assert _paste([_tile(wx=WX + 8)]) == INVALID
    assert _paste([_tile(wy=WY + 4)]) == INVALID
    # shapes
    assert _paste([_tile(tw=18)]) == INVALID                                          # tw % 4
    assert _paste([_tile(tw=0)]) == INVALID
    assert _paste([_tile(th=0)]) == INVALID
    assert _paste([_tile(th=70000)]) == UNSUPPORTED
    assert _paste([_tile()], H=0) == INVALID
    assert _paste([_tile()], W=-1) == INVALID
    assert _paste([_tile()], N=-1) == INVALID
    assert _paste([_tile()], N=65536) == UNSUPPORTED
    assert _paste([_tile(y0=1 << 30)]) == INVALID
    # tile count
    assert _paste([], n=0) == UNSUPPORTED
    assert _paste([_tile(x0=16 * k) for k in range(97)], W=16 * 97) == UNSUPPORTED
    assert _paste([_tile(x0=16 * k) for k in range(96)], W=16 * 96, N=0) == 0
    # one weight pointer only
    assert _paste([_tile(wy=None)]) == INVALID
    assert _paste([_tile(wx=None)]) == INVALID
    # overlap: of the CLIPPED tiles (two tiles that only share pad pixels do not overlap)
    assert _paste([_tile(), _tile(y0=8, x0=8)]) == UNSUPPORTED
    assert b"overlap" in _lib.lib().cgic_last_error()
    assert _paste([_tile(), _tile()]) == UNSUPPORTED
    assert _paste([_tile(y0=-16, x0=-8), _tile(y0=-16, x0=0)], N=0) == 0
    assert _paste([_tile(y0=-8, x0=-8), _tile(y0=-8, x0=0)]) == UNSUPPORTED
    assert _paste([_tile(), _tile(x0=16), _tile(y0=16), _tile(y0=16, x0=16)], N=0) == 0


def test_paste_tiles_is_refused_inside_a_launch_group():
    l = _lib.lib()
    assert l.cgic_group_begin(2, None) == 0
    try:
        assert _paste([_tile()], N=0) == INVALID
    finally:
        l.cgic_group_abort()


def test_paste_tiles_refuses_a_grid_with_a_hole_or_an_overlap():
    H, W = 40, 56                                     # pads to 48 x 64: tiles of 32 -> 32x32, 32x32, 16x32, 16x32
    tiles = highres.tile_grid(48, 64, 32)
    assert tiles == [(0, 0, 32, 32), (0, 32, 32, 32), (32, 0, 16, 32), (32, 32, 16, 32)]
    px = lambda ts: [torch.zeros(1, 3, th, tw) for _, _, th, tw in ts]
    groups = lambda ts: [((th, tw), [i]) for i, (_, _, th, tw) in enumerate(ts)]
    hole = tiles[:3]
    with pytest.raises(ValueError, match="does not cover"):
        highres.paste_tiles(px(hole), (H, W), tiles=hole, groups=groups(hole))
    twice = tiles + [(16, 16, 16, 16)]
    with pytest.raises(ValueError, match="overlap"):
        highres.paste_tiles(px(twice), (H, W), tiles=twice, groups=groups(twice))
    with pytest.raises(ValueError, match="groups must name every tile"):
        highres.paste_tiles(px(tiles), (H, W), tiles=tiles, groups=groups(tiles)[:3])
    # a complete grid passes the geometry checks and reaches the device check (there is no CPU fallback)
    with pytest.raises(RuntimeError, match="HIP"):
        highres.paste_tiles(px(tiles), (H, W), tiles=tiles, groups=groups(tiles))
    with pytest.raises(ValueError, match="image-major"):
        highres.paste_tiles([torch.zeros(2, 3, 32, 32), torch.zeros(1, 3, 16, 32)], (H, W), tile=32)
    with pytest.raises(ValueError, match="multiple of 4"):
        cg.to_frames(torch.zeros(1, 3, 8, 10))


def test_decompress_tiled_batch_keeps_its_signature_defaults():
    import inspect
    p = inspect.signature(highres.decompress_tiled_batch).parameters
    assert p["decode"].default is None and p["frames"].default is False
    assert list(p)[:6] == ["tiled_list", "codec", "concurrent", "check", "chain", "decoder"]
    assert hasattr(highres.TiledCall, "paste") and cg.paste_tiles is highres.paste_tiles and cg.to_frames is highres.to_frames


def test_paste_tiles_op_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        px = [torch.empty(4, 3, 32, 32, device="cuda"), torch.empty(4, 3, 16, 32, device="cuda")]
        out = torch.ops.cgic.paste_tiles(px, 40, 56, 2, 32, True, False)
        assert tuple(out.shape) == (2, 3, 40, 56) and out.dtype == torch.float32 and out.device.type == "cuda"
        fr = torch.ops.cgic.paste_tiles(px, 40, 56, 2, 32, False, True)
        assert tuple(fr.shape) == (2, 40, 56, 3) and fr.dtype == torch.uint8
