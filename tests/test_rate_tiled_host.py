"""CPU: the host side of rate control for tiled images -- the medium axis of a set of tile shapes (tiled_settings), the
vectorised rank search against the loop it restates, choose on a TiledRateCurve with the unpadded-pixel accounting, and the
argument validation of cgic_rate_curve_tiles (which runs before anything touches a device)."""
import ctypes

import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, highres, rate


def _shapes(H, W, tile=768):
    """distinct (h16, w16) of the tiles of an HxW image, in the order the tiling driver groups them"""
    (left, right, top, bottom), _ = highres.compute_padding(H, W)
    tiles = highres.tile_grid(H + top + bottom, W + left + right, tile)
    by = {}
    for _, _, th, tw in tiles:
        by.setdefault((th, tw), []).append(1)
    order = sorted(by.items(), key=lambda kv: -len(kv[1]) * kv[0][0] * kv[0][1])
    return [(th // 16, tw // 16) for (th, tw), _ in order]


def test_shapes_of_the_two_images():
    assert sorted(_shapes(1356, 2040)) == sorted([(48, 48), (48, 32), (37, 48), (37, 32)])
    assert sorted(_shapes(800, 1040)) == sorted([(48, 48), (48, 17), (2, 48), (2, 17)])


@pytest.mark.parametrize("c", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("hw", [(1356, 2040), (800, 1040)])
def test_tiled_settings(hw, c):
    shapes = [h * w for h, w in _shapes(*hw)]
    mediums, ranks = cg.tiled_settings(shapes, c)
    M = mediums.numel()
    assert mediums.dtype == torch.float64 and ranks.dtype == torch.int64 and tuple(ranks.shape) == (len(shapes), M)
    assert 1 <= M <= 65536
    m = mediums.tolist()
    # strictly ascending, inside the open interval of the curve's mode: medium > 0 and fine = 1 - coarse - medium > 0
    assert all(a < b for a, b in zip(m, m[1:]))
    assert m[0] > 0.0 and 1.0 - c - m[-1] > 0.0
    want_mode = 0 if c > 0 else 1
    for s, n16 in enumerate(shapes):
        row = ranks[s].tolist()
        # every entry is the router's own rank for that shape (one foreign call each: the slow form, here on purpose)
        for j in range(M):
            assert row[j] == cg.router_ranks(c, m[j], n16)[1], (s, j)
        assert set(row) == {k for k, _ in rate.reachable_ranks(n16, c)}
    assert all(_lib.lib().cgic_router_mode(c, v) == want_mode for v in m)


@pytest.mark.parametrize("c", [0.0, 0.05, 0.1, 0.3, 0.9])
@pytest.mark.parametrize("n16", [1, 34, 96, 816, 1776, 2304])
def test_vectorised_rank_search_equals_the_loop(n16, c):
    K, m = rate.reachable_ranks_vec(n16, c)
    # the loop side: the scalar search (the specification), one rank at a time -- reachable_ranks is a view of the vectorised one
    loop = [(k, v) for k in range(4 * n16 + 1) for v in [cg.ratio_for_rank(k, n16, c)] if v is not None]
    assert K.tolist() == [k for k, _ in loop]
    assert m.tolist() == [v for _, v in loop]                       # the same float64, bit for bit
    ok, k = rate._curve_ranks_vec(c, m, n16)
    assert bool(ok.all()) and torch.equal(k, K)


def test_unpadded_pixel_accounting_and_choose():
    # two images of 100x70 pixels, each cut into tiles of 64x64 and 48x64 (padded 112x80 -> the tiles hold more pixels than the image)
    H, W = 100, 70
    nb = torch.zeros((2, 3, 5), dtype=torch.int64)
    nb[0, :, 2] = torch.tensor([900, 700, 500])
    nb[0, :, 1] = torch.tensor([0, 50, 150])
    nb[1, :, 2] = torch.tensor([800, 650, 300])
    mediums = torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64)
    ranks = torch.tensor([[2, 3, 5], [1, 2, 3]])
    curve = cg.TiledRateCurve(nb, None, 0.1, mediums, ranks, [(4, 4), (3, 4)], H * W)
    assert curve.bytes.tolist() == [[900, 750, 650], [800, 650, 300]]
    # TiledImage.bpp(): sum(bpp_tile * tw * th) / W / H with bpp_tile = bytes_tile * 8 / (th * tw) -- the tile pixels cancel
    tiles = [(0, 0, 64, 64), (64, 0, 48, 64)]
    per_tile_bytes = [400, 350]                                     # image 0 at setting 1: 750 bytes
    bits = sum((b * 8 / (th * tw)) * tw * th for b, (_, _, th, tw) in zip(per_tile_bytes, tiles))
    assert abs(curve.bpp[0, 1].item() - bits / W / H) < 1e-12
    assert curve.bpp[0, 1].item() == 750 * 8 / (H * W)
    assert curve.batch_bpp.tolist() == [(900 + 800) * 8 / (2 * H * W), (750 + 650) * 8 / (2 * H * W), (650 + 300) * 8 / (2 * H * W)]
    assert curve.candidates == [(0.1, 0.1), (0.1, 0.2), (0.1, 0.3)] and curve.modes == [0, 0, 0]
    bb = curve.batch_bpp.tolist()
    assert cg.choose(curve, bb[1] + 1e-9) == (1, True)
    assert cg.choose(curve, 10.0) == (0, True)
    assert cg.choose(curve, 1e-6) == (2, False)
    k, f = cg.choose(curve, 700 * 8 / (H * W), per="image")
    assert k.tolist() == [2, 1] and f.tolist() == [True, True]
    bad = nb.clone()
    bad[1, 2] = -1
    with pytest.raises(KeyError):
        cg.TiledRateCurve(bad, None, 0.1, mediums, ranks, [(4, 4), (3, 4)], H * W)


def _tile(h16=4, w16=4, k_c=2, shape=0, image=0, off=(0, 0, 0, 0, 0), reserved=0):
    return _lib.RateTile(h16, w16, k_c, shape, image, reserved, *off)


def _call(tiles=None, coarse=0.1, N=1, S=1, M=8, count=None, T=None, table=True, ws=0x2000, ptrs=None, tiles_dev=0x3000, ranks=0x4000,
          out=0x5000):
    coder = cg.HuffmanCoding({str(i): torch.tensor([float(1 + i)]) for i in range(16)})
    tiles = [_tile()] if tiles is None else tiles
    arr = (_lib.RateTile * max(len(tiles), 1))(*tiles)
    cnt = (ctypes.c_int64 * 5)(*(count if count is not None else (16, 64, 256, 16, 64)))
    p = [0x10000] * 5 if ptrs is None else ptrs
    return _lib.lib().cgic_rate_curve_tiles(coder.table.handle if table else None, *p, cnt, arr, tiles_dev, len(tiles) if T is None else T, N,
                                            coarse, ranks, S, M, out, None, ws, None)


def test_argument_validation_before_any_launch():
    E, U = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    for i in range(5):
        p = [0x10000] * 5
        p[i] = None
        assert _call(ptrs=p) == E
    assert _call(table=False) == E and _call(tiles_dev=None) == E and _call(ranks=None) == E and _call(out=None) == E
    assert _call(ws=None) == E and b"workspace" in _lib.lib().cgic_last_error()
    assert _call(ws=0x2004) == E
    assert _call(coarse=-0.1) == E and _call(coarse=float("nan")) == E
    assert _call(M=0) == E and _call(S=0) == E and _call(N=0) == E and _call(T=-1) == E
    assert _call(M=65537) == U and _call(S=17) == U and _call(T=65536) == U
    # descriptors
    assert _call([_tile(h16=64, w16=64, k_c=410)], count=[1 << 20] * 5) == U and b"LDS" in _lib.lib().cgic_last_error()
    assert _call([_tile(h16=0)]) == E
    assert _call([_tile(k_c=3)]) == E and b"k_coarse" in _lib.lib().cgic_last_error()       # round(16 * 0.1) == 2
    assert _call([_tile(k_c=2)], coarse=0.0) == E
    assert _call([_tile(shape=1)]) == E and _call([_tile(image=1)]) == E and _call([_tile(reserved=1)]) == E
    assert _call([_tile(), _tile(h16=2, k_c=1)]) == E and b"two shapes" in _lib.lib().cgic_last_error()
    for i in range(5):
        off = [0] * 5
        off[i] = 1                                                  # one element past the end of its buffer
        assert _call([_tile(off=off)]) == E and b"outside its buffer" in _lib.lib().cgic_last_error()
        off[i] = -1
        assert _call([_tile(off=off)]) == E
    assert _call([_tile(off=[1 << 62] * 5)]) == E


def test_workspace_bytes():
    l = _lib.lib()
    own = l.cgic_rate_curve_tiles_workspace_bytes(6, 1000, 0)
    given = l.cgic_rate_curve_tiles_workspace_bytes(6, 1000, 1)
    assert given >= 6 * 16 and given % 256 == 0 and own == given + 6 * 1000 * 5 * 4
    assert l.cgic_rate_curve_tiles_workspace_bytes(0, 10, 1) == 0 and l.cgic_rate_curve_tiles_workspace_bytes(6, 65537, 1) == 0
