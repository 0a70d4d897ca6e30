"""GPU: every entry point of the library is bound once in Python and reached two ways -- a class method (or a model function) and
a torch.ops.cgic op; HotCall and TiledCall share one buffer builder.  Both ways give the same bits, at the smallest shapes that
have more than one image, a non-square latent and every grain: B=2, image 64x96, latent 16x24."""
import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import highres, model as cgmodel, rate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B, H, W = 2, 64, 96
h, w = H // 4, W // 4


@pytest.fixture(scope="module")
def kit():
    """one quantiser, codec and input set for the module (read-only)"""
    rng = np.random.default_rng(5)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    with torch.no_grad():
        vq.embedding.weight.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.float32)))
    codec = cg.GrainCodec(vq.embedding_counter, vq.embedding.weight.detach())
    x = torch.from_numpy(rng.random((B, 3, H, W), dtype=np.float32)).to(DEV)
    e8, e16 = cg.entropy_maps(x)
    ind = torch.from_numpy(rng.integers(0, 1024, (B, h, w))).to(DEV)
    heads = [torch.from_numpy(rng.integers(0, 1024, (B, h // k, w // k))).to(DEV) for k in (4, 2, 1)]
    return {"rng": rng, "vq": vq, "codec": codec, "table": codec.huffman.table.handle.value, "x": x, "e8": e8, "e16": e16, "ind": ind,
            "heads": heads}


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("ratio, mode", [((0.1, 0.8), 0), ((1.0, 0.0), 4)])
def test_compress_and_decompress_ops_equal_the_codec(kit, ratio, mode):
    """mode 0 writes all five streams; mode 4 (everything coarse) leaves streams unwritten: nbytes -1 on both sides"""
    codec, table = kit["codec"], kit["table"]
    masks, _, _, got_mode = cg.TripleGrainFixedEntropyRouter(*ratio, per_image=True)(kit["e16"], kit["e8"], want_gate=False)
    assert got_mode == mode
    comp = codec.compress(kit["ind"], masks, mode)
    data, nbytes = torch.ops.cgic.compress_streams(kit["ind"], *masks, mode, table, None)
    assert torch.equal(nbytes, comp.nbytes) and tuple(data.shape) == tuple(comp.data.shape)
    assert (int(nbytes.min()) == -1) == (mode == 4)
    assert cg.CompressedBatch(data, nbytes, mode, h, w).to_host() == comp.to_host()
    for decoder in ("latency", "throughput"):
        ind, dmasks, zq, status = codec.decompress(comp, decoder=decoder)
        out = torch.ops.cgic.decompress_streams(data, nbytes, h, w, mode, table, codec.codebook, decoder)
        assert int(status.abs().max()) == 0
        assert _same(out, (ind, *dmasks, zq, status))


def test_histogram_rides_on_the_op_as_on_the_codec(kit):
    masks = cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)(kit["e16"], kit["e8"], want_gate=False)[0]
    h1, h2, h3 = (torch.zeros(1024, dtype=torch.int64, device=DEV) for _ in range(3))
    kit["codec"].compress(kit["ind"], masks, 0, hist=h1)
    torch.ops.cgic.compress_streams(kit["ind"], *masks, 0, kit["table"], h2)
    torch.ops.cgic.index_histogram(kit["ind"], h3)
    assert torch.equal(h1, h2) and torch.equal(h1, h3) and int(h1.sum()) == B * h * w


@pytest.mark.parametrize("coder", ["huffman", "binary"])
def test_stream_ops_equal_the_coders(kit, coder):
    rng = np.random.default_rng(9)
    if coder == "huffman":
        c, sym = kit["codec"].huffman, torch.from_numpy(rng.integers(0, 1024, 100)).to(DEV)
    else:
        c, sym = cg.BinaryCoding(), torch.from_numpy(rng.integers(0, 2, 100).astype(np.int32)).to(DEV)
    table = c.table.handle.value
    want = c.encode_to_bytes(sym)
    out, nbytes = torch.ops.cgic.encode_stream(sym, table)
    n = int(nbytes.item())
    assert bytes(out[:n].cpu().numpy().tobytes()) == want and len(want) > 1
    buf = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)
    buf[:n] = out[:n]
    syms, count = torch.ops.cgic.decode_stream(buf, n, table)
    assert syms[:int(count.item())].cpu().tolist() == c.decode_bytes(want)


def test_blend_ops_equal_the_model_functions_in_place(kit):
    rng = np.random.default_rng(13)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to(DEV)
    m = lambda *s: torch.from_numpy(rng.integers(0, 2, s).astype(np.int32)).to(DEV)
    a, b = t(2, 8, 16, 24), t(2, 8, 16, 24)
    masks = [m(2, 1, 4, 6), m(2, 1, 8, 12), m(2, 1, 16, 24)]
    want = torch.ops.cgic.decoder_blend_medium(a, b, masks[1], masks[2])
    hh = a.clone()
    assert cgmodel.decoder_blend_medium(hh, b, masks[1:], out=hh) is hh and torch.equal(hh, want)
    assert torch.equal(cgmodel.decoder_blend_medium(a, b, masks[1:]), want)
    want = torch.ops.cgic.decoder_blend_fine(a, b, *masks)
    hh = a.clone()
    assert cgmodel.decoder_blend_fine(hh, b, masks, out=hh) is hh and torch.equal(hh, want)
    assert torch.equal(cgmodel.decoder_blend_fine(a, b, masks), want)


def test_rate_ops_equal_the_rate_functions_given_the_codec(kit):
    codec, table, (ic, im, jf), e16, e8 = kit["codec"], kit["table"], kit["heads"], kit["e16"], kit["e8"]
    curve = rate.rate_curve(codec, ic, im, jf, e16, e8, 0.1)
    assert torch.equal(torch.ops.cgic.rate_curve(ic, im, jf, e16, e8, 0.1, table), curve.nbytes)
    cand = [(0.1, 0.8), (0.25, 0.25), (0.0, 0.4)]
    tab = rate.rate_table(codec, ic, im, jf, e16, e8, cand, per_image=True)
    assert torch.equal(torch.ops.cgic.rate_table(ic, im, jf, e16, e8, [c for c, _ in cand], [m for _, m in cand], True, table), tab.nbytes)
    budget = torch.full((1,), int(curve.bytes.sum(dim=0).median()), dtype=torch.int64, device=DEV)
    r = rate.route_to_bpp(codec, ic, im, jf, e16, e8, 0.1, budget=budget)
    out = torch.ops.cgic.route_to_bpp(ic, im, jf, e16, e8, 0.1, budget, table)
    assert _same(out, (*r.masks, r.ind, r.choice)) and r.rank in curve.ranks


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("full", [True, False])
def test_hotcall_equals_the_pipeline(kit, u8, full):
    """the buffer set the shared builder makes: everything wanted, and (decode=False, want_zq=False, want_loss=False)"""
    rng, vq = np.random.default_rng(17), kit["vq"]
    f8 = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    frames = torch.from_numpy(f8).to(DEV)
    # T.ToTensor() of the frames, divided on the host (a correctly rounded fp32 division, as ToTensor's): the fp32 form of the same input
    x = torch.from_numpy(np.ascontiguousarray((f8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))).to(DEV)
    z = torch.from_numpy(rng.standard_normal((2, 4, 16, 16), dtype=np.float32)).to(DEV)
    kw = {} if full else dict(decode=False, want_zq=False, want_loss=False)
    out = cg.pipeline.HotCall(vq, 0.1, 0.8, 2, 64, 64, u8=u8, **kw)(frames if u8 else x, z)
    ref = cg.HotPathPipeline(vq, 0.1, 0.8).run(x, z, decode=full)[0]
    torch.cuda.synchronize()
    assert out["mode"] == ref["mode"] and torch.equal(out["e8"], ref["e8"]) and torch.equal(out["e16"], ref["e16"])
    assert _same(out["mask"], ref["mask"]) and torch.equal(out["ind"], ref["ind"])
    assert out["comp"].to_host() == ref["comp"].to_host()
    assert (out["x"] is None) if not u8 else torch.equal(out["x"], x)
    if full:
        assert torch.equal(out["z_q"], ref["z_q"]) and torch.equal(out["loss"], ref["loss"])
        (i0, m0, q0, s0), (i1, m1, q1, s1) = out["dec"], ref["dec"]
        assert torch.equal(i0, i1) and _same(m0, m1) and torch.equal(q0, q1) and int(s0.abs().max()) == 0 == int(s1.abs().max())
    else:
        assert out["z_q"] is None and out["loss"] is None and out["dec"] is None


@pytest.mark.parametrize("decode", [True, False])
def test_tiledcall_equals_the_chained_tiled_driver(kit, decode):
    """80x112 at tile 64: four shape groups (64x64, 64x48, 16x64, 16x48), one tile each"""
    from control_gic_amd.quantize import vq_forward_route
    rng, vq, codec = np.random.default_rng(19), kit["vq"], kit["codec"]
    tH, tW, tile = 80, 112, 64
    tc = highres.TiledCall(vq, 0.1, 0.8, 1, tH, tW, frequency=codec.huffman, decode=decode, tile=tile)
    assert len(tc.groups) >= 3
    zs = [torch.from_numpy(rng.standard_normal((len(idxs), 4, th // 4, tw // 4), dtype=np.float32)).to(DEV) for (th, tw), idxs in tc.groups]
    zmap = {(th, tw): z for ((th, tw), _), z in zip(tc.groups, zs)}

    def encode(tiles):
        e8, e16 = cg.entropy_maps(tiles)
        _, _, ind, mask, _, mode = vq_forward_route(zmap[tuple(tiles.shape[2:])], vq.embedding.weight, 0.25, True, e16, e8, 0.1, 0.8,
                                                    per_image=True, pixels=tiles)
        return ind, mask, mode

    x = torch.from_numpy((rng.integers(0, 256, (1, 3, tH, tW)) / 255.0).astype(np.float32)).to(DEV)
    got = tc(x, zs)
    ref = highres.compress_tiled(x, encode, codec, tile=tile, chain=True)
    torch.cuda.synchronize()
    assert got.tiles == ref.tiles and got.streams() == ref.streams() and got.bpp() == ref.bpp()
    if decode:
        assert len(tc.decoded) == len(tc.groups) and all(int(d[3].abs().max()) == 0 for d in tc.decoded)
        dref, _ = highres.decompress_tiled(ref, codec, chain=True)
        for ((_, idxs), (dind, dmask, dzq, _)) in zip(tc.groups, tc.decoded):
            for j, i in enumerate(idxs):
                assert torch.equal(dind[j:j + 1], dref[i][0]) and _same([m[j:j + 1] for m in dmask], dref[i][1]) and torch.equal(dzq[j:j + 1], dref[i][2])
    else:
        assert tc.decoded is None
