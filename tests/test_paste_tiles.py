"""GPU: the way out of the tiling driver -- cgic_paste_tiles (ABI 13) and what is built on it -- against the reference's loop.

The expected values are always inference_high_resolution.py:248-255 (accumulate tile * weights and the weights, divide, clamp, unpad)
followed by write_images' conversion (:103), restated on CPU tensors below: never the GPU's torch ops, never the kernel under test.
Comparison is by value with equal NaN positions (the sign of a zero is not pinned)."""
import functools

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, highres

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- the reference's loop on the CPU ---------------------------------------------------------------------------------------
def loop_reference(tile_px, H, W, tile, weighted=True):
    """tile_px: per tile (row-major) a CPU fp32 [N,3,th,tw] -> (rec [N,3,H,W] fp32, frames uint8 [N,H,W,3] numpy)"""
    (left, right, top, bottom), _ = highres.compute_padding(H, W)
    tiles = highres.tile_grid(H + top + bottom, W + left + right, tile)
    N = tile_px[0].shape[0]
    rec = torch.zeros(N, 3, H + top + bottom, W + left + right)
    contrib = torch.zeros_like(rec)
    for (y, x, th, tw), p in zip(tiles, tile_px):
        wts = highres.gaussian_weights(tw, th) if weighted else torch.ones(1, 3, th, tw, dtype=torch.float64)
        rec[:, :, y:y + th, x:x + tw] += p * wts                        # :248
        contrib[:, :, y:y + th, x:x + tw] += wts                        # :249
    rec /= contrib                                                      # :253
    rec = rec.clamp(0, 1)                                               # :254
    rec = rec[:, :, top:top + H, left:left + W].contiguous()            # :255
    with np.errstate(invalid="ignore"):
        frames = (255 * rec.permute(0, 2, 3, 1).numpy()).astype(np.uint8)   # write_images, :103
    return rec, frames


def geometry(H, W, tile):
    (left, right, top, bottom), _ = highres.compute_padding(H, W)
    tiles = highres.tile_grid(H + top + bottom, W + left + right, tile)
    return top, left, tiles, highres._shape_groups(tiles)


def group_batches(tile_px, groups):
    """per-tile CPU [N,3,th,tw] -> per shape group the image-major device batch [N*T,3,th,tw]"""
    N = tile_px[0].shape[0]
    return [torch.stack([tile_px[i][n] for n in range(N) for i in idxs]).to(DEV) for _, idxs in groups]


PLANT = [0.0, 1.0, 1 / 255, 127 / 255, 128 / 255, 254 / 255, -0.0, float("inf")]


@functools.lru_cache(maxsize=None)
def case(H, W, tile, N):
    """seeded tile pixels in [-0.2, 1.2] with planted exact values, and the loop's results (computed once, never modified)"""
    top, left, tiles, groups = geometry(H, W, tile)
    g = torch.Generator().manual_seed(1000 * H + W)
    px = []
    for (_, _, th, tw) in tiles:
        p = torch.rand(N, 3, th, tw, generator=g) * 1.4 - 0.2
        flat = p.view(-1)
        at = torch.randperm(flat.numel(), generator=g)[:3 * len(PLANT)]
        flat[at] = torch.tensor(PLANT * 3)
        px.append(p)
    expect = {w: loop_reference(px, H, W, tile, w) for w in (True, False)}
    return dict(top=top, left=left, tiles=tiles, groups=groups, px=px, expect=expect)


def descriptors(batches, c, N, weighted):
    out = []
    for ((th, tw), idxs), b in zip(c["groups"], batches):
        wx = highres.tile_weight_factors(tw, 0, b.device).data_ptr() if weighted else None
        wy = highres.tile_weight_factors(th, 1, b.device).data_ptr() if weighted else None
        T, per = len(idxs), 3 * th * tw
        for k, i in enumerate(idxs):
            out.append(_lib.PasteTile(b.data_ptr() + 4 * k * per, T * per, wx, wy, c["tiles"][i][0] - c["top"], c["tiles"][i][1] - c["left"], th, tw))
    return out


def raw_paste(desc, N, H, W, f32, u8):
    with torch.cuda.device(0):
        _lib.call("cgic_paste_tiles", N, H, W, len(desc), (_lib.PasteTile * len(desc))(*desc), _lib.ptr(f32), _lib.ptr(u8),
                  _lib.current_stream(torch.device(DEV, 0)))


def same(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    b = b.cpu().numpy() if torch.is_tensor(b) else b
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- 1. equality with the loop ----------------------------------------------------------------------------------------------
SMALL = [(40, 56, 32, 1),      # four tiles, two shapes
         (17, 33, 16, 2),      # odd pads 7/8: misaligned fp32 rows, 99-byte uint8 rows
         (48, 64, 768, 3)]     # one tile, no pad


def _run(c, H, W, tile, N, weighted, mode):
    batches = group_batches(c["px"], c["groups"])
    if mode == "both":                                   # (one launch writes both outputs: the C entry point)
        f32 = torch.full((N, 3, H, W), 9.0, device=DEV)
        u8 = torch.full((N, H, W, 3), 77, dtype=torch.uint8, device=DEV)
        raw_paste(descriptors(batches, c, N, weighted), N, H, W, f32, u8)
        return f32, u8
    out = highres.paste_tiles(batches, (H, W), N=N, weighted=weighted, frames=mode == "u8", tile=tile)
    return (out, None) if mode == "f32" else (None, out)


@pytest.mark.parametrize("mode", ["f32", "u8", "both"])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("H,W,tile,N", SMALL)
def test_paste_equals_the_loop(H, W, tile, N, weighted, mode):
    c = case(H, W, tile, N)
    rec, frames = c["expect"][weighted]
    f32, u8 = _run(c, H, W, tile, N, weighted, mode)
    if f32 is not None:
        assert same(f32, rec), f"{int((f32.cpu() != rec).sum())} fp32 values differ from the loop"
    if u8 is not None:
        assert same(u8, frames), f"{int((u8.cpu().numpy() != frames).sum())} bytes differ from the loop"


def test_weights_do_not_cancel_in_the_loop():
    """what makes the tests above tests of the arithmetic: the weighted loop is NOT a plain clamp"""
    c = case(40, 56, 32, 1)
    assert int((c["expect"][True][0] != c["expect"][False][0]).sum()) > 100


def test_paste_equals_the_loop_at_the_real_geometry():
    """2040 x 1356: pad 4/4/2/2, six tiles in four shape groups, weighted, both outputs in one launch"""
    H, W, tile, N = 1356, 2040, 768, 1
    c = case(H, W, tile, N)
    assert [len(ix) for _, ix in c["groups"]] == [2, 2, 1, 1]
    rec, frames = c["expect"][True]
    f32, u8 = _run(c, H, W, tile, N, True, "both")
    assert same(f32, rec) and same(u8, frames)


def test_nan_stays_nan_in_fp32_and_is_zero_in_uint8():
    H, W, tile = 40, 56, 32
    c = case(H, W, tile, 1)
    px = [p.clone() for p in c["px"]]
    px[0][0, 1, 10, 12] = float("nan")
    y, x = 10 - c["top"], 12 - c["left"]
    rec, frames = (v.clone() if torch.is_tensor(v) else v.copy() for v in c["expect"][True])
    rec[0, 1, y, x] = float("nan")
    frames[0, y, x, 1] = 0
    batches = group_batches(px, c["groups"])
    f32 = highres.paste_tiles(batches, (H, W), tile=tile)
    u8 = highres.paste_tiles(batches, (H, W), tile=tile, frames=True)
    assert bool(torch.isnan(f32[0, 1, y, x])) and int(torch.isnan(f32).sum()) == 1
    assert same(f32, rec)                                        # ... and the neighbours are what they were
    assert int(u8[0, y, x, 1]) == 0 and same(u8, frames)
    u8p = highres.paste_tiles(batches, (H, W), tile=tile, frames=True, weighted=False)
    plain = c["expect"][False][1].copy()
    plain[0, y, x, 1] = 0
    assert same(u8p, plain)


# ---- 2. the fixture of the real reference ------------------------------------------------------------------------------------
def test_fixture_of_the_real_reference(golden):
    g = golden("paste")
    H, W = (int(v) for v in g["image_hw"])
    top, left, tiles, groups = geometry(H, W, highres.TILE)
    assert (H, W) == (776, 8) and tiles == [(0, 0, 768, 16), (768, 0, 16, 16)] and list(g["pad"]) == [4, 4, 4, 4]
    px = [torch.from_numpy(g[f"tile{t}"])[None] for t in range(int(g["n_tiles"]))]
    batches = group_batches(px, groups)
    assert same(highres.paste_tiles(batches, (H, W)), g["rec"])
    assert same(highres.paste_tiles(batches, (H, W), frames=True), g["frames"])


# ---- 3. batch and order independence ---------------------------------------------------------------------------------------------
def test_batch_of_three_equals_three_calls_and_order_is_free():
    H, W, tile, N = 17, 33, 16, 3
    c = case(H, W, tile, N)
    batches = group_batches(c["px"], c["groups"])
    whole = highres.paste_tiles(batches, (H, W), N=N, tile=tile)
    whole8 = highres.paste_tiles(batches, (H, W), N=N, tile=tile, frames=True)
    for n in range(N):
        one = [b[n * len(idxs):(n + 1) * len(idxs)].contiguous() for b, (_, idxs) in zip(batches, c["groups"])]
        assert same(highres.paste_tiles(one, (H, W), tile=tile)[0], whole[n])
        assert same(highres.paste_tiles(one, (H, W), tile=tile, frames=True)[0], whole8[n])
    desc = descriptors(batches, c, N, True)
    assert len(desc) == 6
    for perm in ([5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 4, 3]):
        f32 = torch.empty_like(whole)
        u8 = torch.empty_like(whole8)
        raw_paste([desc[i] for i in perm], N, H, W, f32, u8)
        assert same(f32, whole) and same(u8, whole8)


def test_unweighted_paste_undoes_cut_groups():
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 40, 56, generator=g) * 1.4 - 0.2
    pad, tiles, order, batches = highres.cut_groups(x.to(DEV), tile=32)
    back = highres.paste_tiles(batches, (40, 56), tiles=tiles, groups=order, N=2, weighted=False, tile=32)
    assert same(back, x.clamp(0, 1))
    assert same(highres.paste_tiles(batches, (40, 56), N=2, weighted=False, tile=32), x.clamp(0, 1))       # derived geometry: the same


# ---- 4. nothing else is written ----------------------------------------------------------------------------------------------------
def test_guard_bands_and_uncovered_pixels_stay_untouched():
    H, W, tile, N = 17, 33, 16, 2
    c = case(H, W, tile, N)
    rec, frames = c["expect"][True]
    batches = group_batches(c["px"], c["groups"])
    desc = descriptors(batches, c, N, True)
    n32, n8, G32, G8 = N * 3 * H * W, N * H * W * 3, 37, 61           # (odd guards: the outputs start 4- and 1-byte aligned only)
    buf32 = torch.full((G32 + n32 + G32,), 7.0, device=DEV)
    buf8 = torch.full((G8 + n8 + G8,), 0xAB, dtype=torch.uint8, device=DEV)
    f32, u8 = buf32[G32:G32 + n32].view(N, 3, H, W), buf8[G8:G8 + n8].view(N, H, W, 3)
    raw_paste(desc, N, H, W, f32, u8)
    assert same(f32, rec) and same(u8, frames)
    for buf, G, n, v in ((buf32, G32, n32, 7.0), (buf8, G8, n8, 0xAB)):
        assert bool((buf[:G] == v).all()) and bool((buf[G + n:] == v).all()), "written outside the output"
    # the tiles of the first row only: what no tile covers keeps its bytes (tile pixels inside the pad went nowhere)
    buf32.fill_(7.0)
    buf8.fill_(0xAB)
    first_row = [d for d in desc if d.y0 < 0]
    assert 0 < len(first_row) < len(desc)
    rows = max(d.y0 + d.th for d in first_row)
    raw_paste(first_row, N, H, W, f32, u8)
    assert same(f32[:, :, :rows], rec[:, :, :rows]) and same(u8[:, :rows], frames[:, :rows])
    assert bool((f32[:, :, rows:] == 7.0).all()) and bool((u8[:, rows:] == 0xAB).all())
    assert bool((buf32[:G32] == 7.0).all()) and bool((buf32[G32 + n32:] == 7.0).all())
    assert bool((buf8[:G8] == 0xAB).all()) and bool((buf8[G8 + n8:] == 0xAB).all())


# ---- 5. graph capture --------------------------------------------------------------------------------------------------------------
def test_paste_is_capturable_and_replays_on_new_tiles():
    H, W, tile, N = 40, 56, 32, 2
    c = case(H, W, tile, N)
    batches = group_batches(c["px"], c["groups"])
    out = torch.empty(N, 3, H, W, device=DEV)
    out8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device=DEV)
    highres.paste_tiles(batches, (H, W), N=N, tile=tile, out=out)             # eager once: the weight factors are on the device
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # one stream, no forked branches
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        r = highres.paste_tiles(batches, (H, W), N=N, tile=tile, out=out)
        r8 = highres.paste_tiles(batches, (H, W), N=N, tile=tile, out=out8, frames=True)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before, "paste_tiles(out=...) allocated device memory"
        with pytest.raises(RuntimeError, match="outside a graph capture"):
            highres.tile_weight_factors(20, 0, DEV)                            # an extent nobody pasted yet: refused while capturing
    assert r is out and r8 is out8
    # new tile contents in the captured buffers: the replay must paste THEM
    c2 = case(40, 56, 32, 3)
    fresh = [p[:N] * 0.5 + 0.25 for p in c2["px"]]
    for b, nb in zip(batches, group_batches(fresh, c["groups"])):
        b.copy_(nb)
    out.fill_(5.0)
    out8.fill_(5)
    graph.replay()
    torch.cuda.synchronize()
    rec, frames = loop_reference(fresh, H, W, tile)
    assert same(out, rec) and same(out8, frames)
    assert same(highres.paste_tiles(batches, (H, W), N=N, tile=tile), out)      # replay == eager


def test_tiled_call_paste_uses_its_own_geometry():
    H, W, tile, N = 40, 56, 32, 2
    c = case(H, W, tile, N)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    call = highres.TiledCall(vq, 0.1, 0.8, N, H, W, decode=False, tile=tile)
    assert call.groups == c["groups"]
    batches = group_batches(c["px"], c["groups"])
    assert same(call.paste(batches), c["expect"][True][0])
    out8 = torch.empty(N, H, W, 3, dtype=torch.uint8, device=DEV)
    assert call.paste(batches, out=out8, frames=True) is out8 and same(out8, c["expect"][True][1])


# ---- 6. batched decode ---------------------------------------------------------------------------------------------------------------
def test_decompress_tiled_batch_decodes_once_per_group_and_pastes():
    H, W, tile, N = 40, 56, 32, 2
    rng = np.random.default_rng(0)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    vq.embedding.weight.data.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.float32)))
    codec = cg.GrainCodec(vq.embedding_counter, vq.embedding.weight)
    router = cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)
    g = torch.Generator().manual_seed(11)

    def encode(batch):
        e8, e16 = cg.entropy_maps(batch)
        mask, _, _, mode = router(e16, e8)
        z = torch.randn(batch.shape[0], 4, batch.shape[-2] // 4, batch.shape[-1] // 4, generator=g).to(DEV)
        return vq.indices(z), mask, mode

    x = torch.rand(N, 3, H, W, generator=g).to(DEV)
    tiled = highres.compress_tiled_batch(x, encode, codec, tile=tile)
    calls = []

    def pixels_of(zq):
        # nearest x4 upsample of three latent channels, scaled out of [0, 1] by exact operations (x2 is exact: a fused and an
        # unfused multiply-add round alike, so the device and the CPU make the same tile pixels)
        return zq[:, :3].repeat_interleave(4, dim=-2).repeat_interleave(4, dim=-1) * 2.0 + 0.5

    def f(zq, masks):
        calls.append(tuple(zq.shape))
        return pixels_of(zq).contiguous()

    plain = highres.decompress_tiled_batch(tiled, codec)
    per_image, rec = highres.decompress_tiled_batch(tiled, codec, decode=f)
    assert sorted(calls) == sorted([(N * 2, 4, 8, 8), (N * 2, 4, 4, 8)]), "decode must be called once per shape group on the whole batch"
    calls.clear()
    per_image8, frames = highres.decompress_tiled_batch(tiled, codec, decode=f, frames=True)
    assert len(calls) == 2
    assert tuple(rec.shape) == (N, 3, H, W) and rec.dtype == torch.float32
    assert tuple(frames.shape) == (N, H, W, 3) and frames.dtype == torch.uint8
    for n in range(N):
        assert all(torch.equal(a[2], b[2]) and torch.equal(a[0], b[0]) for a, b in zip(plain[n], per_image[n]))
        want, want8 = loop_reference([pixels_of(t[2].cpu()) for t in per_image[n]], H, W, tile)
        assert float(want.min()) == 0.0 and float(want.max()) == 1.0             # (the stand-in does leave [0, 1])
        assert same(rec[n:n + 1], want) and same(frames[n:n + 1], want8)


# ---- 7. the untiled exit ---------------------------------------------------------------------------------------------------------------
def test_to_frames_is_write_images():
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(2, 3, 16, 20, generator=g) * 1.4 - 0.2).clamp(0, 1)
    x[0, 0, 0, :4] = torch.tensor([0.0, 1.0, 128 / 255, 254 / 255])
    want = (255 * x.permute(0, 2, 3, 1).detach().cpu().numpy()).astype(np.uint8)
    got = cg.to_frames(x.to(DEV))
    assert same(got, want)
    out = torch.empty(2, 16, 20, 3, dtype=torch.uint8, device=DEV)
    assert cg.to_frames(x.to(DEV), out=out) is out and same(out, want)
    raw = torch.rand(2, 3, 16, 20, generator=g) * 1.4 - 0.2                    # unclamped input: to_frames clamps (inference.py:163)
    assert same(cg.to_frames(raw.to(DEV)), (255 * raw.clamp(0, 1).permute(0, 2, 3, 1).numpy()).astype(np.uint8))
