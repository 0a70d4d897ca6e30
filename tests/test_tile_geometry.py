"""CPU: the one tile geometry of the tiled path (highres.tile_geometry and what is built on it).  Bytes, pictures and bpp all follow the
order of the shape groups, tie-break included, so the order is pinned here against hand-worked values and against a restatement of
the grouping every caller used to carry itself."""
import pytest
import torch

from control_gic_amd import highres
from control_gic_amd.codec import CompressedBatch


def _groups_as_the_callers_wrote_them(tiles):
    by_shape = {}
    for i, (_, _, th, tw) in enumerate(tiles):
        by_shape.setdefault((th, tw), []).append(i)
    return sorted(by_shape.items(), key=lambda kv: -len(kv[1]) * kv[0][0] * kv[0][1])


GRID48 = [(0, 0, 32, 32), (0, 32, 32, 16), (32, 0, 16, 32), (32, 32, 16, 16)]
CASES = [
    # 2040x1356: padded 1360x2048, 2 x 3 tiles; the two-tile groups first, the larger of them in front
    (1356, 2040, 768, (4, 4, 2, 2),
     [(0, 0, 768, 768), (0, 768, 768, 768), (0, 1536, 768, 512), (768, 0, 592, 768), (768, 768, 592, 768), (768, 1536, 592, 512)],
     [((768, 768), [0, 1]), ((592, 768), [3, 4]), ((768, 512), [2]), ((592, 512), [5])]),
    # (32,16) and (16,32) tie on count x area: the first appearance in row-major order decides
    (48, 48, 32, (0, 0, 0, 0), GRID48, [((32, 32), [0]), ((32, 16), [1]), ((16, 32), [2]), ((16, 16), [3])]),
    # ragged, with an odd centred pad: 1 column (all of it right), 15 rows (7 above, 8 below)
    (33, 47, 32, (0, 1, 7, 8), GRID48, [((32, 32), [0]), ((32, 16), [1]), ((16, 32), [2]), ((16, 16), [3])]),
    (16, 16, 768, (0, 0, 0, 0), [(0, 0, 16, 16)], [((16, 16), [0])]),
]


@pytest.mark.parametrize("H,W,tile,pad,tiles,groups", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in CASES])
def test_tile_geometry_is_pad_grid_and_groups_largest_first(H, W, tile, pad, tiles, groups):
    got = highres.tile_geometry(H, W, tile)
    assert got == (pad, tiles, groups)
    # == the pieces every caller used to put together itself
    p, _ = highres.compute_padding(H, W)
    grid = highres.tile_grid(H + p[2] + p[3], W + p[0] + p[1], tile)
    assert got == (p, grid, _groups_as_the_callers_wrote_them(grid)) and highres._shape_groups(grid) == got[2]
    areas = [len(idxs) * th * tw for (th, tw), idxs in got[2]]
    assert areas == sorted(areas, reverse=True)


def test_tile_geometry_default_tile_is_the_references():
    assert highres.tile_geometry(1356, 2040) == highres.tile_geometry(1356, 2040, 768) and highres.TILE == 768


def test_placed_tiles_in_launch_order():
    pad, tiles, groups = highres.tile_geometry(33, 47, 32)
    left, _, top, _ = pad
    assert list(highres._placed(tiles, groups, top, left)) == [(0, 0, 1, -7, 0, 32, 32), (1, 0, 1, -7, 32, 32, 16), (2, 0, 1, 25, 0, 16, 32),
                                                               (3, 0, 1, 25, 32, 16, 16)]
    pad, tiles, groups = highres.tile_geometry(1356, 2040)
    got = list(highres._placed(tiles, groups, 2, 4))
    assert got[:4] == [(0, 0, 2, -2, -4, 768, 768), (0, 1, 2, -2, 764, 768, 768), (1, 0, 2, 766, -4, 592, 768), (1, 1, 2, 766, 764, 592, 768)]
    assert got[4:] == [(2, 0, 1, -2, 1532, 768, 512), (3, 0, 1, 766, 1532, 592, 512)]


def test_groups_must_name_every_tile_once_under_its_own_shape():
    _, tiles, groups = highres.tile_geometry(48, 48, 32)
    highres._check_groups(tiles, groups, "x")
    highres._check_groups(tiles, groups[::-1], "x")                      # any order of the groups
    for bad in (groups[:3], groups + [((16, 16), [3])], [((32, 32), [0]), ((16, 32), [1]), ((32, 16), [2]), ((16, 16), [3])]):
        with pytest.raises(ValueError, match="what: groups must name every tile once, under its own shape"):
            highres._check_groups(tiles, bad, "what")
    top, left, t2, g2 = highres._resolve_geometry(48, 48, 32, None, None, "x")
    assert (top, left, t2, g2) == (0, 0, tiles, groups)
    assert highres._resolve_geometry(48, 48, 32, list(tiles), None, "x")[3] == groups        # the caller's tiles: grouped the same way
    with pytest.raises(ValueError, match="does not cover"):
        highres._resolve_geometry(48, 48, 32, tiles[:3], None, "x")
    assert highres._resolve_geometry(48, 48, 32, tiles[:3], None, "x", cover=False)[2] == tiles[:3]


def test_assemble_tiled_marks_shared_buffers_only_where_they_last():
    N, (pad, tiles, order) = 2, highres.tile_geometry(40, 48, 32)
    groups = []
    for (th, tw), idxs in order:
        B, per = N * len(idxs), (th // 4) * (tw // 4)
        comp = CompressedBatch(torch.arange(B * 5 * 8, dtype=torch.uint8).view(B, 5, 8), torch.arange(B * 5, dtype=torch.int32).view(B, 5), 0, th // 4, tw // 4)
        groups.append((idxs, comp, (torch.arange(B * per), [torch.arange(B).view(B, 1, 1, 1)] * 3, 0)))
    kept = highres.assemble_tiled((40, 48), pad, tiles, groups, N)
    loose = highres.assemble_tiled((40, 48), pad, tiles, groups, N, whole=False)
    assert [t._whole[1:] for t in kept] == [(0, N), (1, N)] and all(t._whole[0] is groups for t in kept)
    assert not any(hasattr(t, "_whole") for t in loose)
    for a, b in zip(kept, loose):                                            # the same views either way
        assert a.tiles == b.tiles == tiles and a.pad == b.pad == pad and a.shape_groups() == order
        for (ia, ca, (inda, ma, _)), (ib, cb, (indb, mb, _)) in zip(a.groups, b.groups):
            assert ia == ib and torch.equal(ca.data, cb.data) and torch.equal(ca.nbytes, cb.nbytes) and torch.equal(inda, indb)
            assert ca.data.data_ptr() == cb.data.data_ptr() and all(torch.equal(p, q) for p, q in zip(ma, mb))
    # image n holds tiles [n T, (n + 1) T) of every group
    for n, t in enumerate(kept):
        for (idxs, comp, (ind, masks, _)), (_, whole, (wind, _, _)) in zip(t.groups, groups):
            T = len(idxs)
            assert torch.equal(comp.data, whole.data[n * T:(n + 1) * T]) and masks[0].flatten().tolist() == list(range(n * T, (n + 1) * T))
            assert torch.equal(ind, wind.view(N * T, -1)[n * T:(n + 1) * T].reshape(-1))
