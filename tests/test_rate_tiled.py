"""GPU: rate control for tiled high-resolution images (cgic_rate_curve_tiles, rate_curve_tiled, compress_tiled_to_bpp) --
against the CPU oracle at settings spread over the medium axis, against the library's own single-shape curve at every tile and
setting, end to end on the stand-in model of test_rate_control.py, and the error paths."""
import ctypes

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, highres
from oracle import cgic_oracle as orc
from oracle.content_families import families

from test_rate_control import FREQ, _model, _vq
from test_rate_curve import _oracle_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _content(name, n, H, W, seed):
    """n images of HxW from a content family (made at the next multiple of 8 rows / columns, which the families need, and cropped)"""
    x = families(n=n, H=(H + 7) // 8 * 8, W=(W + 7) // 8 * 8, seed=seed)[name]
    return np.ascontiguousarray(x[:, :, :H, :W])


def _groups(x, vq, cb, seed, oracle=True):
    """x [N,3,H,W] numpy -> (order, the shape groups rate_curve_tiled takes, per group what the oracle needs): the tiles cut as the
    tiling driver cuts them, reference-order maps, random encoder heads"""
    rng = np.random.default_rng(seed)
    N = x.shape[0]
    pad, grid, order, batches = highres.cut_groups(torch.from_numpy(x).to(DEV))
    groups, host = [], []
    for ((th, tw), idxs), batch in zip(order, batches):
        B = batch.shape[0]
        assert B == N * len(idxs)
        heads = [rng.standard_normal((B, 4, th // s, tw // s)).astype(np.float32) for s in (16, 8, 4)]
        e8, e16 = cg.entropy_maps(batch, reference_order=True)
        inds = cg.grain_indices(vq, *[torch.from_numpy(h).to(DEV) for h in heads])
        images = [n for n in range(N) for _ in idxs]
        groups.append((*inds, e16, e8, images))
        if oracle:
            oind = [orc.vq(h, cb)[2].reshape(B, h.shape[2], h.shape[3]) for h in heads]
            host.append((e16.cpu().numpy(), e8.cpu().numpy(), oind, images))
    return order, groups, host


def _oracle_image_sizes(host, htab, c, m, N):
    """[N][5]: per image the sum over its tiles of the oracle's stream sizes at (c, m), every tile routed on its own thresholds"""
    want = np.zeros((N, 5), np.int64)
    for e16n, e8n, oind, images in host:
        sizes, _ = _oracle_sizes(e16n, e8n, oind, htab, c, m)
        for b, n in enumerate(images):
            want[n] += np.asarray(sizes[b], np.int64)
    return want.tolist()


@pytest.mark.parametrize("coarse", [0.1, 0.0])
@pytest.mark.parametrize("fam_name", ["smooth8", "flat_edges"])
@pytest.mark.parametrize("H,W", [(1356, 2040), (800, 1040)])
def test_tiled_curve_against_oracle(H, W, fam_name, coarse):
    x = _content(fam_name, 1, H, W, seed=H + 5)
    rng = np.random.default_rng(H)
    cb = rng.standard_normal((1024, 4)).astype(np.float32)
    vq = _vq(cb)
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    order, groups, host = _groups(x, vq, cb, seed=W)
    assert len(order) == 4 and sum(len(ix) for _, ix in order) == (6 if H == 1356 else 4)      # four tile shapes
    counter = vq.usage_counter.clone()
    curve = cg.rate_curve_tiled(codec, groups, coarse, image_hw=(H, W))
    assert torch.equal(vq.usage_counter, counter)
    M = curve.mediums.numel()
    T = sum(len(ix) for _, ix in order)
    assert tuple(curve.nbytes.shape) == (1, M, 5) and tuple(curve.tile_nbytes.shape) == (T, M, 5) and tuple(curve.ranks.shape) == (4, M)
    assert curve.shapes == [(th // 16, tw // 16) for (th, tw), _ in order]
    htab = orc.HuffmanTable(FREQ)
    picks = sorted({int(j) for j in np.linspace(0, M - 1, 28).round()})
    assert len(picks) >= 24 and picks[0] == 0 and picks[-1] == M - 1
    nb = curve.nbytes.numpy()
    wrong = []
    for j in picks:
        c, m = curve.candidates[j]
        assert c == coarse
        for s, (h16, w16) in enumerate(curve.shapes):
            assert cg.router_ranks(c, m, h16 * w16)[1] == int(curve.ranks[s, j])
        want = _oracle_image_sizes(host, htab, c, m, 1)
        if nb[:, j].tolist() != want:
            wrong.append((j, m, nb[:, j].tolist(), want))
    # both ends of the axis: medium 0 and fine 0
    assert len(curve.ends.candidates) == 2
    for ci, (c, m) in enumerate(curve.ends.candidates):
        want = _oracle_image_sizes(host, htab, c, m, 1)
        if curve.ends.nbytes[ci].tolist() != want:
            wrong.append(("end", m, curve.ends.nbytes[ci].tolist(), want))
    assert not wrong, (fam_name, coarse, len(wrong), wrong[:3])
    # the reference's accounting: bits over the pixels of the UNPADDED image
    assert curve.bpp[0, picks[3]].item() == int(nb[0, picks[3]].sum()) * 8 / (H * W)
    # coarse patches per tile, as the oracle's router counts them
    at = 0
    for e16n, e8n, oind, images in host:
        omc = orc.router(e16n, e8n, coarse, curve.mediums[M // 2].item(), per_image=True)[0]
        if coarse > 0:
            assert curve.n_coarse[at:at + len(images)].tolist() == [int(omc[b].sum()) for b in range(len(images))]
        at += len(images)


@pytest.mark.parametrize("coarse", [0.1, 0.0])
def test_tiles_equal_the_single_shape_curve_in_any_order_and_company(coarse):
    N, H, W = 2, 1356, 2040
    x = np.concatenate([_content("smooth8", 1, H, W, seed=3), _content("flat_edges", 1, H, W, seed=4)])
    rng = np.random.default_rng(77)
    cb = rng.standard_normal((1024, 4)).astype(np.float32)
    vq = _vq(cb)
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    order, groups, _ = _groups(x, vq, cb, seed=8, oracle=False)
    curve = cg.rate_curve_tiled(codec, groups, coarse, image_hw=(H, W), ends=False)
    M = curve.mediums.numel()
    # every tile, every setting: the single-shape curve of its group at the rank of its shape class
    at = 0
    for s, g in enumerate(groups):
        single = cg.rate_curve(codec, *g[:5], coarse, ranks=())
        B = len(g[5])
        want = single.nbytes[:, curve.ranks[s].to(DEV)]                             # [B, M, 5]
        got = curve.tile_nbytes[at:at + B]
        assert torch.equal(got, want), (s, (got != want).nonzero()[:5].tolist())
        assert curve.tile_shape[at:at + B] == [s] * B and curve.tile_image[at:at + B] == g[5]
        at += B
    assert at == 12
    # the fold: int64 sums over the tiles of each image
    tn = curve.tile_nbytes.cpu().to(torch.int64)
    for n in range(N):
        mine = [t for t, i in enumerate(curve.tile_image) if i == n]
        assert torch.equal(curve.nbytes[n], tn[mine].sum(dim=0))

    # permuted descriptors: the groups reversed and cut into one group per tile, the tiles of the two images interleaved
    singles = []
    for ind_c, ind_m, ind_f, e16, e8, images in reversed(groups):
        for b in reversed(range(len(images))):
            singles.append((ind_c[b:b + 1], ind_m[b:b + 1], ind_f[b:b + 1], e16[b:b + 1], e8[b:b + 1], [images[b]]))
    perm = cg.rate_curve_tiled(codec, singles, coarse, image_hw=(H, W), ends=False)
    assert perm.tile_image != curve.tile_image and perm.shapes == curve.shapes[::-1]
    assert torch.equal(perm.mediums, curve.mediums) and torch.equal(perm.ranks, curve.ranks.flip(0))
    assert torch.equal(perm.nbytes, curve.nbytes)
    # company: each image alone gives its rows of the shared call
    for n in range(N):
        alone = [tuple(t[[b for b, i in enumerate(g[5]) if i == n]] for t in g[:5]) + ([0] * (len(g[5]) // N),) for g in groups]
        one = cg.rate_curve_tiled(codec, alone, coarse, image_hw=(H, W), ends=False)
        assert torch.equal(one.mediums, curve.mediums) and torch.equal(one.nbytes[0], curve.nbytes[n])


def _total_bytes(tiled):
    return sum(sum(len(v) for v in s.values()) for s in tiled.streams())


def test_compress_tiled_to_bpp_end_to_end():
    model = _model()
    H, W = 1356, 2040
    x = torch.from_numpy(_content("smooth8", 1, H, W, seed=11)).to(DEV)
    counter = model.quantize.usage_counter.clone()
    params = model.encoder.router_config["params"]
    c0 = params["coarse_grain_ratio"]
    with torch.no_grad():
        _, _, _, full = model.compress_tiled_to_bpp(x, 1e9)
    assert isinstance(full, cg.TiledRateCurve) and full.mediums.numel() > 9000
    every = full.batch_bpp.tolist() + full.ends.batch_bpp.tolist()
    lo, hi = min(every), max(every)
    codec = model._cgic_codec
    htab = orc.HuffmanTable(FREQ)
    # the maps the call routes on: the same tiles, the same entropy call
    pad, grid, order, batches = highres.cut_groups(x)
    maps = [cg.entropy_maps(b, reference_order=True) for b in batches]
    for target, want_fits in ((lo + 0.37 * (hi - lo), True), (lo * 0.5, False), (hi * 2, True)):
        with torch.no_grad():
            tiled, bpp, (c, m), curve = model.compress_tiled_to_bpp(x, target)
        assert isinstance(tiled, highres.TiledImage) and c == c0 and curve.fits == want_fits
        assert torch.equal(curve.nbytes, full.nbytes) and torch.equal(curve.mediums, full.mediums)
        # the curve's entry of the chosen setting (or of the chosen end)
        if curve.chosen is not None:
            assert curve.candidates[curve.chosen] == (c, m)
            entry_bytes, entry_bpp = int(curve.bytes[0, curve.chosen]), curve.bpp[0, curve.chosen].item()
        else:
            ci = curve.ends.candidates.index((c, m))
            entry_bytes, entry_bpp = int(curve.ends.bytes[ci, 0]), curve.ends.bpp[ci, 0].item()
        assert bpp == entry_bpp == entry_bytes * 8 / (H * W)
        assert _total_bytes(tiled) == entry_bytes
        # TiledImage.bpp() sums bytes * 8 / (th * tw) * tw * th over six tiles in float64: each term is within two roundings of
        # bytes * 8, the sum within six more -- 8 * 2^-53 relative, far inside 1e-12
        print(f"target {target:.6f} bpp: {bpp:.6f} ({target - bpp:.6f} under), medium ratio {m!r}, fits {curve.fits}")
        assert abs(tiled.bpp() - entry_bpp) <= 1e-12 * entry_bpp
        if curve.fits:
            assert bpp <= target
            assert not [v for v in every if bpp < v <= target]        # no setting, ends included, between it and the target
        else:
            assert bpp == lo
        # every tile's five streams: the oracle's router on the same maps at that ratio, the oracle's coder on the indices
        streams = tiled.streams()
        for (idxs, comp, (ind, masks, mode)), (e8, e16) in zip(tiled.groups, maps):
            omc, omm, omf, _, omode = orc.router(e16.cpu().numpy(), e8.cpu().numpy(), c, m, per_image=True)
            assert omode == mode
            indn = ind.view(len(idxs), comp.h, comp.w).cpu().numpy()
            for k, i in enumerate(idxs):
                for got_mask, want_mask in zip(masks, (omc, omm, omf)):
                    assert np.array_equal(got_mask[k, 0].cpu().numpy(), want_mask[k, 0])
                assert streams[i] == orc.compress_image(indn[k], omc[k, 0], omm[k, 0], omf[k, 0], omode, htab), (target, i)
        # both decoders return the indices that were compressed
        for decoder in ("latency", "throughput"):
            per_tile, _ = highres.decompress_tiled(tiled, codec, decoder=decoder)
            for idxs, comp, (ind, masks, mode) in tiled.groups:
                for k, i in enumerate(idxs):
                    assert torch.equal(per_tile[i][0][0], ind.view(len(idxs), comp.h, comp.w)[k])
    assert torch.equal(model.quantize.usage_counter, counter) and int(model.quantize.usage_hist.abs().sum()) == 0
    # N images of one size: ONE ratio pair for all of them, picked on the batch
    x2 = torch.from_numpy(np.concatenate([_content("smooth8", 1, 800, 1040, seed=5), _content("flat_edges", 1, 800, 1040, seed=6)])).to(DEV)
    with torch.no_grad():
        _, _, _, f2 = model.compress_tiled_to_bpp(x2, 1e9)
        target = float(f2.batch_bpp.median())
        out, bpps, (c, m), cur = model.compress_tiled_to_bpp(x2, target)
    assert len(out) == 2 and cur.fits and cur.chosen is not None and bpps == cur.bpp[:, cur.chosen].tolist()
    assert [_total_bytes(t) for t in out] == cur.bytes[:, cur.chosen].tolist()
    assert sum(bpps) / 2 <= target and cur.batch_bpp[cur.chosen].item() == max(v for v in cur.batch_bpp.tolist() + cur.ends.batch_bpp.tolist() if v <= target)
    model.quantize.train()
    with pytest.raises(RuntimeError):
        model.compress_tiled_to_bpp(x2, 0.5)
    model.quantize.eval()


def _small(vq, B=2, H=64, W=64):
    rng = np.random.default_rng(9)
    x = torch.from_numpy(families(n=B, H=H, W=W, seed=2)["smooth8"]).to(DEV)
    heads = [torch.from_numpy(rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32)).to(DEV) for s in (16, 8, 4)]
    e8, e16 = cg.entropy_maps(x, reference_order=True)
    return [t.clone() for t in cg.grain_indices(vq, *heads)], e16, e8


def test_error_paths_write_nothing():
    rng = np.random.default_rng(9)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    inds, e16, e8 = _small(vq)
    l = _lib.lib()
    T, N, S, M = 2, 2, 1, 8
    k_c = cg.router_ranks(0.1, 0.4, 16)[0]
    good = [_lib.RateTile(4, 4, k_c, 0, b, 0, 16 * b, 64 * b, 256 * b, 16 * b, 64 * b) for b in range(T)]
    count = (ctypes.c_int64 * 5)(32, 128, 512, 32, 128)
    ranks = torch.tensor([[7, 8, 9, 20, 30, 40, 50, 64]], dtype=torch.int32, device=DEV)
    image_nb = torch.full((N, M, 5), -777, dtype=torch.int64, device=DEV)
    tile_nb = torch.full((T, M, 5), -777, dtype=torch.int32, device=DEV)
    ws = torch.full((l.cgic_rate_curve_tiles_workspace_bytes(T, M, 1),), 0xAB, dtype=torch.uint8, device=DEV)

    def call(tiles, M_=M, ranks_=ranks):
        arr = (_lib.RateTile * len(tiles))(*tiles)
        dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        rc = l.cgic_rate_curve_tiles(codec.huffman.table.handle, *[_lib.ptr(t) for t in (*inds, e16, e8)], count, arr, _lib.ptr(dev), len(tiles), N,
                                     0.1, _lib.ptr(ranks_), S, M_, _lib.ptr(image_nb), _lib.ptr(tile_nb), _lib.ptr(ws), _lib.current_stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return int((image_nb != -777).sum()) == 0 and int((tile_nb != -777).sum()) == 0 and int((ws != 0xAB).sum()) == 0

    # a tile beyond n8 = 12288 (its parts would not lie inside the buffers either: the shape is refused first)
    big = _lib.RateTile(64, 64, round(4096 * 0.1), 0, 1, 0, 0, 0, 0, 0, 0)
    assert call([good[0], big]) == _lib.ERR_UNSUPPORTED and b"LDS" in l.cgic_last_error() and untouched()
    # a descriptor whose fine indices end one tile past the buffer
    off = _lib.RateTile(4, 4, k_c, 0, 1, 0, 16, 64, 512 - 255, 16, 64)
    assert call([good[0], off]) == _lib.ERR_INVALID and b"outside its buffer" in l.cgic_last_error() and untouched()
    # more settings than the limit
    assert call(good, M_=65537) == _lib.ERR_UNSUPPORTED and untouched()
    # ... and the same call with nothing wrong writes everything, equal to the single-shape curve
    assert call(good) == _lib.OK
    single = cg.rate_curve(codec, *inds, e16, e8, 0.1, ranks=())
    assert torch.equal(tile_nb, single.nbytes[:, ranks[0].long()])
    assert torch.equal(image_nb, tile_nb.to(torch.int64))               # one tile per image
    # a rank outside 0 .. n8 of the tile: negative entries, the image's five sizes -1
    bad_ranks = ranks.clone()
    bad_ranks[0, 3] = 65
    assert call(good, ranks_=bad_ranks) == _lib.OK
    assert int(image_nb[:, 3].max()) == -1 and int(image_nb[:, 3].min()) == -1 and int(tile_nb[:, 3].max()) < -1
    keep = [j for j in range(M) if j != 3]
    assert torch.equal(tile_nb[:, keep], single.nbytes[:, ranks[0].long()][:, keep])


def test_symbol_outside_the_table_is_a_key_error():
    rng = np.random.default_rng(9)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    inds, e16, e8 = _small(vq)
    good = cg.rate_curve_tiled(codec, [(*inds, e16, e8, [0, 1])], 0.1)
    assert int(good.nbytes.min()) >= 0
    inds[1].view(2, -1)[1, :] = 1024                                    # every medium symbol of image 1's tile
    l = _lib.lib()
    mediums, ranks = cg.tiled_settings([16], 0.1)
    M = mediums.numel()
    desc = (_lib.RateTile * 2)(*[_lib.RateTile(4, 4, 2, 0, b, 0, 16 * b, 64 * b, 256 * b, 16 * b, 64 * b) for b in range(2)])
    dev = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(DEV)
    image_nb = torch.empty((2, M, 5), dtype=torch.int64, device=DEV)
    ws = torch.empty(l.cgic_rate_curve_tiles_workspace_bytes(2, M, 0), dtype=torch.uint8, device=DEV)      # tile_nbytes inside the workspace
    ranks_dev = ranks.to(torch.int32).to(DEV)
    _lib.call("cgic_rate_curve_tiles", codec.huffman.table.handle, *[_lib.ptr(t) for t in (*inds, e16, e8)], (ctypes.c_int64 * 5)(32, 128, 512, 32, 128),
              desc, _lib.ptr(dev), 2, 2, 0.1, _lib.ptr(ranks_dev), 1, M, _lib.ptr(image_nb), None, _lib.ptr(ws), _lib.current_stream())
    nb = image_nb.cpu()
    assert torch.equal(nb[0], good.nbytes[0])                           # the other image is untouched by its neighbour's symbol
    neg = (nb[1] < 0).any(dim=1)
    assert int(neg.sum()) > 0 and torch.equal(nb[1][neg], torch.full((int(neg.sum()), 5), -1, dtype=torch.int64))
    assert torch.equal(nb[1][~neg], good.nbytes[1][~neg]) and torch.equal(neg, good.nbytes[1, :, 1] > 0)
    with pytest.raises(KeyError):
        cg.rate_curve_tiled(codec, [(*inds, e16, e8, [0, 1])], 0.1)
