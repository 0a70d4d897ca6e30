"""GPU: the partition map (cgic_partition_map / draw.py / highres.partition_tiles) against CPU expectations -- the fixture of the REAL
draw_triple_grain_256res, the restated cell loops (small shapes) and the closed form (large shapes) of tests/partition_ref.py, which
tests/test_partition_host.py holds to each other.  Nothing here is compared with GPU torch operations or with the kernel itself."""
import functools

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, draw, highres
import partition_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(t, a):
    """bit equality of a device tensor and a numpy array (NaNs by their bits)"""
    got = t.cpu().numpy()
    if got.dtype == np.float32:
        return got.shape == a.shape and np.array_equal(got.view(np.uint32), np.ascontiguousarray(a, dtype=np.float32).view(np.uint32))
    return got.shape == a.shape and got.dtype == a.dtype and np.array_equal(got, a)


def masks_dev(m):
    return [dev(np.asarray(v, dtype=np.int32)) for v in m]


def lines_of(H, W, ind):
    return np.stack([ref.line_mask(H, W, ind[b]) for b in range(ind.shape[0])])


def raw_call(src, tiles, N, H, W, f32=None, u8=None):
    arr = (_lib.PartitionTile * len(tiles))(*tiles)
    _lib.call("cgic_partition_map", src.data_ptr(), int(src.dtype == torch.uint8), N, H, W, len(tiles), arr,
              None if f32 is None else f32.data_ptr(), None if u8 is None else u8.data_ptr(), torch.cuda.current_stream().cuda_stream)


# ---- 1. the fixture of the real function ---------------------------------------------------------------------------------------------
def _fixture_cases(g):
    for si in range(3):
        for ri in range(7):
            key = f"s{si}_r{ri}"
            yield key, g[f"s{si}_x"], [g[f"{key}_{m}"].astype(np.int32) for m in ("mc", "mm", "mf")], g[f"{key}_ind"].astype(np.int64)
    yield "malformed", g["s1_x"], None, g["malformed_ind"]
    yield "ragged", g["ragged_x"], None, g["ragged_ind"]


def test_fixture_pictures_through_every_entry_and_every_conversion(golden):
    g = golden("partition")
    for key, frames, mask, ind in _fixture_cases(g):
        B, H, W, _ = frames.shape
        pic, fr = ref.decode_pic(g[f"{key}_pic"]), g[f"{key}_frames"]
        x, x8 = dev(ref.to_unit(frames)), dev(frames)
        # the reference's function: in place, returns its argument
        y = x.clone()
        assert cg.draw_triple_grain_256res(y, dev(ind)) is y and same(y, pic), key
        assert same(cg.draw_triple_grain_256res(x.clone(), dev(ind.astype(np.int32))), pic)          # any integer dtype
        if mask is None:
            continue
        m = masks_dev(mask)
        assert same(cg.partition_map(x, m), pic), key                                                  # fp32 -> fp32
        assert same(cg.partition_map(x, m, frames=True), fr), key                                      # fp32 -> uint8
        assert same(cg.partition_map(x8, m, frames=True), fr), key                                     # uint8 -> uint8
        assert same(cg.partition_map(x8, m), pic), key                                                 # uint8 -> fp32
        assert same(x, ref.to_unit(frames)) and same(x8, frames), "the source was modified"
        assert same(torch.ops.cgic.partition_map(x, m[0], m[1], m[2], False), pic)
        # the raw C call: both outputs in one launch, masks form and indices form; then in place
        ind_d = dev(ind)
        for tile in (_lib.PartitionTile(m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(), None, 1, 0, 0, H, W, 0, 0),
                     _lib.PartitionTile(None, None, None, ind_d.data_ptr(), 1, 0, 0, H, W, ind.shape[1], ind.shape[2])):
            for src in (x, x8):
                o32, o8 = torch.full((B, 3, H, W), 9.0, device=DEV), torch.full((B, H, W, 3), 9, dtype=torch.uint8, device=DEV)
                raw_call(src, [tile], B, H, W, o32, o8)
                assert same(o32, pic) and same(o8, fr), key
        y, y8 = x.clone(), x8.clone()
        assert cg.partition_map(y, m, out=y) is y and same(y, pic)
        assert cg.partition_map(y8, m, frames=True, out=y8) is y8 and same(y8, fr)
        # in place with the OTHER output made in the same launch
        y, o8 = x.clone(), torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
        raw_call(y, [_lib.PartitionTile(m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(), None, 1, 0, 0, H, W, 0, 0)], B, H, W, y, o8)
        assert same(y, pic) and same(o8, fr)


def test_fixture_tiled_pictures(golden):
    g = golden("partition")
    for name in ("t0", "t1"):
        H, W, tile = (int(v) for v in g[f"{name}_hw_tile"])
        pad, tiles, groups = ref.geometry(H, W, tile)
        per_tile = [[g[f"{name}_tile{i}_{m}"].astype(np.int32) for m in ("mc", "mm", "mf")] for i in range(len(tiles))]
        masks = [masks_dev([np.concatenate([per_tile[i][j] for i in idxs]) for j in range(3)]) for _, idxs in groups]
        x8 = dev(g[f"{name}_x"])
        x = dev(ref.to_unit(g[f"{name}_x"]))
        pic, fr = ref.decode_pic(g[f"{name}_pic"]), g[f"{name}_frames"]
        assert same(cg.partition_tiles(x, masks, tile=tile), pic)
        assert same(cg.partition_tiles(x, masks, tile=tile, frames=True), fr)
        assert same(cg.partition_tiles(x8, masks, tile=tile), pic)
        assert same(cg.partition_tiles(x8, masks, tile=tile, frames=True), fr)


# ---- 2. the mask rule --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mask_case(B, H, W, kind):
    rng = np.random.default_rng(B * 1000 + H + W)
    x = (rng.random((B, 3, H, W)) * 1.2 - 0.1).astype(np.float32)
    mc, mm, mf = ref.random_partition(rng, B, H, W)
    if kind == "zero":
        mc, mm, mf = (np.zeros_like(m) for m in (mc, mm, mf))
    elif kind == "overlapping":
        mc, mm, mf = ((rng.random(m.shape) < 0.5).astype(np.int32) for m in (mc, mm, mf))
    elif kind == "wild":
        mc, mm, mf = ((rng.integers(-2, 3, m.shape) * 1000003).astype(np.int32) for m in (mc, mm, mf))
    ind = ref.first_maximum(mc, mm, mf)
    pic = ref.loop_draw(x, ind)
    return x, (mc, mm, mf), ind, pic, ref.to_frames(pic, lines_of(H, W, ind))


@pytest.mark.parametrize("kind", ["partition", "zero", "overlapping", "wild"])
@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (2, 32, 48), (3, 64, 32), (2, 48, 64)])
def test_mask_rule_is_the_first_maximum(B, H, W, kind):
    x, mask, ind, pic, fr = mask_case(B, H, W, kind)
    m = masks_dev(mask)
    assert same(cg.partition_map(dev(x), m), pic)
    assert same(cg.partition_map(dev(x), m, frames=True), fr)
    assert same(cg.grain_map(m), ind)
    assert same(cg.partition_map(dev(x), [v[:, 0] for v in m]), pic)                  # masks without the singleton axis


# ---- 3. the indices form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,gh,gw", [(1, 27, 41, 6, 10), (2, 5, 7, 5, 7), (2, 32, 48, 1, 8), (1, 33, 50, 8, 12), (3, 18, 21, 4, 4), (1, 64, 6, 16, 1)])
def test_indices_form_on_ragged_grids_and_odd_widths(B, H, W, gh, gw):
    rng = np.random.default_rng(H * W + gh)
    x = rng.random((B, 3, H, W)).astype(np.float32)
    for values in ((-1, 0, 1, 2, 3), (0, 1, 2, 1 << 40, (1 << 40) + 1, (1 << 40) + 2, (1 << 32) + 2)):
        ind = rng.choice(np.array(values, dtype=np.int64), (B, gh, gw))
        pic = ref.loop_draw(x, ind)
        y = dev(x)
        assert cg.draw_triple_grain_256res(y, dev(ind)) is y and same(y, pic)
        # every conversion of the indices form through the raw call (uint8 rows of odd width: the byte-store path)
        fr = ref.to_frames(pic, lines_of(H, W, ind))
        x8 = dev(ref.to_frames(x, np.zeros((B, H, W), bool)))
        o32, o8 = torch.empty(B, 3, H, W, device=DEV), torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
        ind_d = dev(ind)
        tile = _lib.PartitionTile(None, None, None, ind_d.data_ptr(), 1, 0, 0, H, W, gh, gw)
        raw_call(dev(x), [tile], B, H, W, o32, o8)
        assert same(o32, pic) and same(o8, fr)
        raw_call(x8, [tile], B, H, W, o32, o8)
        x8n = x8.cpu().numpy()
        pic8 = ref.loop_draw(ref.to_unit(x8n), ind)
        assert same(o32, pic8) and same(o8, ref.to_frames(pic8, lines_of(H, W, ind)))
        assert same(x8, x8n)


def test_draw_takes_the_first_images_of_a_longer_batch_and_refuses_a_grid_finer_than_the_image():
    rng = np.random.default_rng(5)
    x = rng.random((3, 3, 32, 32)).astype(np.float32)
    ind = rng.integers(0, 3, (2, 8, 8))
    want = x.copy()
    want[:2] = ref.loop_draw(x[:2], ind)
    assert same(cg.draw_triple_grain_256res(dev(x), dev(ind)), want)
    with pytest.raises(cg.CgicError) as e:
        cg.draw_triple_grain_256res(dev(x), dev(np.zeros((1, 33, 8), np.int64)))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(IndexError):
        cg.draw_triple_grain_256res(dev(x), dev(np.zeros((4, 8, 8), np.int64)))
    with pytest.raises(ValueError):
        cg.draw_triple_grain_256res(dev(x).permute(0, 1, 3, 2), dev(ind))


# ---- 4. tiled ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiled_case(H, W, tile, N, drawer="loop"):
    rng = np.random.default_rng(H + W + tile + N)
    pad, tiles, groups = ref.geometry(H, W, tile)
    x = rng.random((N, 3, H, W)).astype(np.float32)
    per_tile = [ref.random_partition(rng, N, th, tw) for _, _, th, tw in tiles]                # per tile: masks of the N images
    inds = [ref.first_maximum(*m) for m in per_tile]
    pic, line = ref.tiled_expected(x, inds, pad, tiles, ref.loop_draw if drawer == "loop" else ref.closed_form)
    return {"x": x, "pad": pad, "tiles": tiles, "groups": groups, "per_tile": per_tile, "pic": pic, "line": line, "frames": ref.to_frames(pic, line)}


def group_masks(per_tile, groups, images=None):
    """per shape group the image-major mask buffers [N*T,1,.,.]: image n's tiles of the group, then image n + 1's"""
    out = []
    for _, idxs in groups:
        N = per_tile[idxs[0]][0].shape[0]
        ns = range(N) if images is None else images
        out.append(masks_dev([np.concatenate([per_tile[i][j][n:n + 1] for n in ns for i in idxs]) for j in range(3)]))
    return out


@pytest.mark.parametrize("H,W,tile,N", [(40, 56, 32, 1), (17, 33, 16, 2), (48, 64, 768, 3)])
def test_tiled_map_is_the_per_tile_drawer_on_the_padded_image(H, W, tile, N):
    c = tiled_case(H, W, tile, N)
    masks = group_masks(c["per_tile"], c["groups"])
    x = dev(c["x"])
    x8n = ref.to_frames(c["x"], np.zeros((N, H, W), bool))
    assert same(cg.partition_tiles(x, masks, tile=tile), c["pic"])
    assert same(cg.partition_tiles(x, masks, tile=tile, frames=True), c["frames"])
    pic8, line8 = ref.tiled_expected(ref.to_unit(x8n), [ref.first_maximum(*m) for m in c["per_tile"]], c["pad"], c["tiles"])
    assert same(cg.partition_tiles(dev(x8n), masks, tile=tile), pic8)
    assert same(cg.partition_tiles(dev(x8n), masks, tile=tile, frames=True), ref.to_frames(pic8, line8))
    assert same(x, c["x"])
    y = x.clone()
    assert cg.partition_tiles(y, masks, tile=tile, out=y) is y and same(y, c["pic"])


def test_batch_of_three_equals_three_calls_and_order_is_free():
    H, W, tile, N = 40, 56, 32, 3
    c = tiled_case(H, W, tile, N)
    x = dev(c["x"])
    whole = cg.partition_tiles(x, group_masks(c["per_tile"], c["groups"]), tile=tile)
    assert same(whole, c["pic"])
    for n in range(N):
        one = cg.partition_tiles(x[n:n + 1], group_masks(c["per_tile"], c["groups"], images=[n]), tile=tile)
        assert torch.equal(one[0], whole[n])
    # tiles and groups handed over in another order: the descriptors' order does not matter
    perm = [3, 1, 0, 2]
    tiles = [c["tiles"][i] for i in perm]
    groups = [((th, tw), [perm.index(i) for i in reversed(idxs)]) for (th, tw), idxs in reversed(c["groups"])]
    per_tile = [c["per_tile"][i] for i in perm]
    assert same(cg.partition_tiles(x, group_masks(per_tile, groups), tiles=tiles, groups=groups), c["pic"])


def test_tiles_that_overlap_across_two_launches_are_refused_and_draw_refuses_uint8_frames():
    H, W, tile, N = 160, 176, 16, 1
    c = tiled_case(H, W, tile, N, "closed")
    tiles = list(c["tiles"]) + [c["tiles"][0]]                      # tile 110 lies on tile 0: they land in different launches
    groups = [((16, 16), list(range(111)))]
    masks = group_masks(c["per_tile"] + [c["per_tile"][0]], groups)
    out = torch.zeros(N, 3, H, W, device=DEV)
    with pytest.raises(ValueError, match="overlap"):
        cg.partition_tiles(dev(c["x"]), masks, tiles=tiles, groups=groups, out=out)
    assert float(out.abs().max()) == 0.0                            # refused before anything was drawn
    with pytest.raises(ValueError, match="fp32"):
        cg.draw_triple_grain_256res(torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int64, device=DEV))


def test_more_tiles_than_one_launch_takes_are_split():
    H, W, tile, N = 160, 176, 16, 2                                 # 10 x 11 = 110 tiles > 84
    c = tiled_case(H, W, tile, N, "closed")
    assert len(c["tiles"]) == 110 > draw.MAX_TILES
    assert same(cg.partition_tiles(dev(c["x"]), group_masks(c["per_tile"], c["groups"]), tile=tile), c["pic"])
    assert same(cg.partition_tiles(dev(c["x"]), group_masks(c["per_tile"], c["groups"]), tile=tile, frames=True), c["frames"])


# ---- 5. the real geometry once ------------------------------------------------------------------------------------------------------
def test_real_geometry_six_tiles_in_four_shapes():
    H, W = 1356, 2040
    c = tiled_case(H, W, 768, 1, "closed")
    assert len(c["tiles"]) == 6 and len(c["groups"]) == 4
    masks = group_masks(c["per_tile"], c["groups"])
    assert same(cg.partition_tiles(dev(c["x"]), masks), c["pic"])
    assert same(cg.partition_tiles(dev(c["x"]), masks, frames=True), c["frames"])


# ---- 6. guard bands, uncovered pixels, special values ------------------------------------------------------------------------------
def test_guard_bands_and_uncovered_pixels_stay_untouched():
    H, W, tile, N = 40, 56, 32, 2
    c = tiled_case(H, W, tile, N)
    G32, G8, n32, n8 = 1024, 4096, N * 3 * H * W, N * H * W * 3
    buf32 = torch.full((G32 + n32 + G32,), 7.0, device=DEV)
    buf8 = torch.full((G8 + n8 + G8,), 0xAB, dtype=torch.uint8, device=DEV)
    out32, out8 = buf32[G32:G32 + n32].view(N, 3, H, W), buf8[G8:G8 + n8].view(N, H, W, 3)
    masks = group_masks(c["per_tile"], c["groups"])
    cg.partition_tiles(dev(c["x"]), masks, tile=tile, out=out32)
    cg.partition_tiles(dev(c["x"]), masks, tile=tile, out=out8, frames=True)
    assert same(out32, c["pic"]) and same(out8, c["frames"])
    assert bool((buf32[:G32] == 7.0).all()) and bool((buf32[G32 + n32:] == 7.0).all())
    assert bool((buf8[:G8] == 0xAB).all()) and bool((buf8[G8 + n8:] == 0xAB).all())
    # a grid with a hole: the pixels no tile covers keep what the outputs held
    keep = [0, 1, 3]
    tiles = [c["tiles"][i] for i in keep]
    groups = [((32, 32), [0, 1]), ((16, 32), [2])]
    per_tile = [c["per_tile"][i] for i in keep]
    out32.fill_(7.0)
    out8.fill_(0xAB)
    cg.partition_tiles(dev(c["x"]), group_masks(per_tile, groups), tiles=tiles, groups=groups, out=out32)
    cg.partition_tiles(dev(c["x"]), group_masks(per_tile, groups), tiles=tiles, groups=groups, out=out8, frames=True)
    left, _, top, _ = c["pad"]
    y, x0, th, tw = c["tiles"][2]
    hole = np.zeros((H, W), bool)
    hole[max(y - top, 0):y - top + th, max(x0 - left, 0):x0 - left + tw] = True
    want32, want8 = c["pic"].copy(), c["frames"].copy()
    want32[:, :, hole], want8[:, hole] = 7.0, 0xAB
    assert hole.any() and same(out32, want32) and same(out8, want8)
    with pytest.raises(ValueError, match="does not cover"):
        cg.partition_tiles(dev(c["x"]), group_masks(per_tile, groups), tiles=tiles, groups=groups)        # no `out`: nothing to keep


def test_special_values_follow_the_stated_conversion_and_lines_are_lines_whatever_the_source_holds():
    B, H, W = 2, 32, 48
    rng = np.random.default_rng(8)
    x = (rng.random((B, 3, H, W)) * 3 - 1).astype(np.float32)                       # values outside [0, 1] too
    special = np.array([np.nan, np.inf, -np.inf, -0.0, -1.0, 1.0, 0.0, 255.5 / 255, 1e-45, -1e-45], dtype=np.float32)
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, 1500, replace=False)] = rng.choice(special, 1500)
    mask = ref.random_partition(rng, B, H, W)
    ind = ref.first_maximum(*mask)
    line = lines_of(H, W, ind)
    pic = ref.loop_draw(x, ind)
    assert np.isnan(x[np.repeat(line[:, None], 3, 1)]).any() and np.isnan(pic).any() and np.isinf(pic).any()
    m = masks_dev(mask)
    assert same(cg.partition_map(dev(x), m), pic)                                     # NaN, +-Inf, -0.0 bit for bit off the lines
    fr = ref.to_frames(pic, line)
    assert same(cg.partition_map(dev(x), m, frames=True), fr)
    got = cg.partition_map(dev(x), m, frames=True).cpu().numpy()
    assert (got[line] == 1).all()
    off = ~np.repeat(line[..., None], 3, -1)
    src = x.transpose(0, 2, 3, 1)
    assert (got[off & np.isnan(src)] == 0).all() and (got[off & (src == np.inf)] == 255).all() and (got[off & (src < 0)] == 0).all()


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------
def test_partition_map_and_tiled_call_partition_are_capturable():
    B, H, W = 2, 32, 48
    x, mask, ind, pic, fr = mask_case(B, H, W, "partition")
    xd, m = dev(x), masks_dev(mask)
    out, out8 = torch.empty(B, 3, H, W, device=DEV), torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)
    tH, tW, tile, N = 40, 56, 32, 2
    c = tiled_case(tH, tW, tile, N)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    call = highres.TiledCall(vq, 0.1, 0.8, N, tH, tW, decode=False, tile=tile)
    assert call.groups == c["groups"]
    for t, gm in zip(call._buf, group_masks(c["per_tile"], c["groups"])):              # this call's own mask buffers, filled by hand
        for dst, srcm in zip(t["mask"], gm):
            dst.copy_(srcm)
    tx, tout = dev(c["x"]), torch.empty(N, 3, tH, tW, device=DEV)
    cg.partition_map(xd, m, out=out)                                                   # eager once
    assert same(call.partition(tx), c["pic"]) and same(call.partition(tx, frames=True), c["frames"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                      # one stream, a single chain
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        r = cg.partition_map(xd, m, out=out)
        r8 = cg.partition_map(xd, m, frames=True, out=out8)
        rt = call.partition(tx, out=tout)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before, "partition_map(out=...) allocated device memory"
    assert r is out and r8 is out8 and rt is tout
    # new pixels and new masks in the captured buffers: the replay must draw THEM
    x2, mask2, ind2, pic2, fr2 = mask_case(B, H, W, "overlapping")
    xd.copy_(dev(x2))
    for dst, srcm in zip(m, masks_dev(mask2)):
        dst.copy_(srcm)
    c2 = tiled_case(tH, tW, tile, 3)
    per_tile2 = [tuple(v[:N] for v in t) for t in c2["per_tile"]]
    for t, gm in zip(call._buf, group_masks(per_tile2, c["groups"])):
        for dst, srcm in zip(t["mask"], gm):
            dst.copy_(srcm)
    tx.copy_(dev(c2["x"][:N]))
    out.fill_(5.0), out8.fill_(5), tout.fill_(5.0)
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, pic2) and same(out8, fr2)
    want, _ = ref.tiled_expected(c2["x"][:N], [ref.first_maximum(*t) for t in per_tile2], c["pad"], c["tiles"])
    assert same(tout, want)


# ---- 8. end to end on the stand-in model ----------------------------------------------------------------------------------------------
def test_compress_save_img_draws_the_routing_that_was_used(tmp_path):
    import test_rate_control as trc
    from oracle.content_families import families
    model = trc._model()
    x = torch.from_numpy(families(n=3, seed=4)["smooth8"]).to(DEV)
    _, _, H, W = x.shape
    with torch.no_grad():
        a, b = tmp_path / "a", tmp_path / "b"
        a.mkdir(), b.mkdir()
        dec0, bpp0, none = model.compress(x[:1], str(a), save_img=False)
        dec1, bpp1, pmap = model.compress(x[:1], str(b), save_img=True)
        assert none is None and bpp0 == bpp1 and torch.equal(dec0, dec1)
        files = sorted(p.name for p in a.iterdir())
        assert files and files == sorted(p.name for p in b.iterdir())
        assert all((a / f).read_bytes() == (b / f).read_bytes() for f in files)
        # ... equals the CPU drawing of the masks encode() returned for that image alone
        params = model.encoder.router_config["params"]
        had, before = "per_image" in params, params.get("per_image")
        params["per_image"] = True
        try:
            _, _, _, mask, _, _, _ = model.encode(x[:1])
            _, _, _, mask3, _, _, _ = model.encode(x)
        finally:
            if had:
                params["per_image"] = before
            else:
                del params["per_image"]
        ind = ref.first_maximum(*(m.cpu().numpy() for m in mask))
        assert pmap.dtype == torch.float32 and same(pmap, ref.loop_draw(x[:1].cpu().numpy(), ind))
        assert (ind == 0).any() and (ind == 1).any() and (ind == 2).any()
        # the batch
        dec3, bpp3, comp3 = model.compress_batch(x, save_img=True)
        ind3 = ref.first_maximum(*(m.cpu().numpy() for m in mask3))
        assert same(comp3.partition_map, ref.loop_draw(x.cpu().numpy(), ind3))
        decp, bppp, compp = model.compress_batch(x)
        assert compp.partition_map is None and bppp == bpp3 and compp.to_host() == comp3.to_host() and torch.equal(decp, dec3)
        assert model.partition_map is cg.partition_map and model.partition_tiles is cg.partition_tiles
        # what the stock encoder calls grain_indices: the reference's picture of that tensor, for whoever needs it
        bad = torch.cat([m.float().repeat_interleave(k, -2).repeat_interleave(k, -1) for m, k in zip(mask, (4, 2, 1))], dim=-1).permute(0, 3, 1, 2).argmax(dim=1)
        assert tuple(bad.shape) == (1, 1, H // 4)
        assert same(cg.draw_triple_grain_256res(x[:1].clone(), bad), ref.loop_draw(x[:1].cpu().numpy(), bad.cpu().numpy()))


def test_compress_tiled_batch_then_partition_tiles():
    H, W, tile, N = 40, 56, 32, 2
    rng = np.random.default_rng(0)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    vq.embedding.weight.data.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.float32)))
    codec = cg.GrainCodec(vq.embedding_counter, vq.embedding.weight)
    router = cg.TripleGrainFixedEntropyRouter(0.25, 0.5, per_image=True)
    g = torch.Generator().manual_seed(11)

    def encode(batch):
        e8, e16 = cg.entropy_maps(batch)
        mask, _, _, mode = router(e16, e8)
        z = torch.randn(batch.shape[0], 4, batch.shape[-2] // 4, batch.shape[-1] // 4, generator=g).to(DEV)
        return vq.indices(z), mask, mode

    x = torch.rand(N, 3, H, W, generator=g).to(DEV)
    tiled = highres.compress_tiled_batch(x, encode, codec, tile=tile)
    pad, tiles, groups = ref.geometry(H, W, tile)
    inds = [None] * len(tiles)
    for n, t in enumerate(tiled):
        for idxs, _, (_, masks, _) in t.groups:
            for k, i in enumerate(idxs):
                one = ref.first_maximum(*(m[k:k + 1].cpu().numpy() for m in masks))
                inds[i] = one if inds[i] is None else np.concatenate([inds[i], one])
    want, line = ref.tiled_expected(x.cpu().numpy(), inds, pad, tiles)
    assert same(cg.partition_tiles(x, tiled, tile=tile), want)
    assert same(cg.partition_tiles(x, tiled, frames=True), ref.to_frames(want, line))
    # one image of the list on its own, and a single TiledImage
    assert same(cg.partition_tiles(x[1:2], tiled[1]), want[1:2])
    assert same(cg.partition_tiles(x[1:2], [tiled[1]]), want[1:2])
    with pytest.raises(ValueError):
        cg.partition_tiles(x, tiled[:1])
