"""GPU: exact per-ratio rate tables (cgic_rate_table), the grain-index gather and compress_to_bpp -- against the real
reference's file sizes (tests/golden/rate.npz), against the library's own route -> gather -> compress chain, and against the
CPU oracle."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch
from torch import nn

import control_gic_amd as cg
from control_gic_amd import _lib
from oracle import cgic_oracle as orc
from oracle.content_families import families

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
FREQ = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)
# all seven modes: 0, 0, 2, 3, 1, 4, 5, 6
CANDS = [(0.1, 0.8), (0.3, 0.3), (0.2, 0.0), (0.25, 0.75), (0.0, 0.5), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)]


def _vq(cb):
    vq = cg.VectorQuantizer(cb.shape[0], cb.shape[1], beta=0.25).to(DEV).eval()
    vq.embedding.weight.data.copy_(torch.as_tensor(cb))
    vq.usage_counter.copy_(torch.from_numpy(FREQ.astype(np.float32)))
    return vq


def _conv(w, b):
    qc = nn.Conv2d(4, 4, 1).to(DEV)
    with torch.no_grad():
        qc.weight.copy_(torch.as_tensor(w).reshape(4, 4, 1, 1))
        qc.bias.copy_(torch.as_tensor(b))
    return qc


def _chain(codec, inds, e16, e8, c, m, per_image, pixels):
    """the library's own route -> gather -> compress: the sizes cgic_rate_table promises"""
    router = cg.TripleGrainFixedEntropyRouter(c, m, per_image=per_image)
    masks, _, _, mode = router(e16, e8, want_gate=False, pixels=pixels)
    ind = cg.gather_grain_indices(*inds, masks)
    comp = codec.compress(ind, masks, mode)
    return comp.nbytes.clamp(min=0), ind, masks


def test_golden_reference_sizes():
    g = np.load(os.path.join(HERE, "golden", "rate.npz"))
    cand = [tuple(r) for r in g["candidates"]]
    vq = _vq(g["codebook"])
    qc = _conv(g["qc_w"], g["qc_b"])
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    for ii in range(len(g["names"])):
        x = torch.from_numpy(g[f"img{ii}_x"].transpose(2, 0, 1)[None].astype(np.float32) / 255.0).to(DEV)
        e8, e16 = cg.entropy_maps(x)
        heads = [torch.from_numpy(g[f"img{ii}_h{k}"]).to(DEV) for k in "cmf"]
        inds = cg.grain_indices(vq, *heads, quant_conv=qc)
        tab = cg.rate_table(codec, *inds, e16, e8, cand, per_image=True, pixels=x)
        nb = tab.nbytes.cpu().numpy()
        for ci, (c, m) in enumerate(cand):
            masks, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(e16, e8, want_gate=False, pixels=x)
            assert mode == int(g[f"img{ii}_c{ci}_mode"])
            ind = cg.gather_grain_indices(*inds, masks)
            assert np.array_equal(ind[0].cpu().numpy(), g[f"img{ii}_c{ci}_ind"].astype(np.int64)), (ii, ci)
            assert np.array_equal(nb[ci, 0], g[f"img{ii}_c{ci}_sizes"]), (ii, ci, nb[ci, 0], g[f"img{ii}_c{ci}_sizes"])
            assert tab.bpp[ci, 0].item() == g[f"img{ii}_c{ci}_sizes"].sum() * 8 / (256 * 256)


def _case(B, H, W, seed, kind):
    fam = families(n=B, H=H, W=W, seed=seed)
    x = torch.from_numpy(fam["smooth8" if seed % 2 else "flat_edges"]).to(DEV)
    rng = np.random.default_rng(seed)
    heads = [torch.from_numpy(rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32)).to(DEV) for s in (16, 8, 4)]
    if kind == "u8":
        frames = (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        x2, e8, e16 = cg.entropy_maps_u8(frames)
        return heads, e16, e8, frames
    e8, e16 = cg.entropy_maps(x)
    return heads, e16, e8, (x if kind == "f32" else None)


@pytest.mark.parametrize("B,H,W,per_image,kind", [
    (1, 256, 256, True, "f32"), (16, 256, 256, True, "f32"), (16, 256, 256, False, "u8"), (64, 256, 256, True, "u8"),
    (64, 256, 256, False, "f32"), (1, 768, 768, True, "f32"), (3, 64, 96, True, "none"), (3, 64, 96, False, "f32"),
    (16, 256, 256, True, "none")])
def test_rate_table_equals_route_gather_compress(B, H, W, per_image, kind):
    rng = np.random.default_rng(B + H)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    qc = _conv(rng.standard_normal((4, 4)).astype(np.float32) * 0.5, rng.standard_normal(4).astype(np.float32) * 0.1)
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    heads, e16, e8, px = _case(B, H, W, B + W, kind)
    if B == 64 and not per_image:
        assert _lib.lib().cgic_router_refine_in_lds(B, H // 16, W // 16, 0) == 0       # the launch-chain path
    inds = cg.grain_indices(vq, *heads, quant_conv=qc)
    counter = vq.usage_counter.clone()
    tab = cg.rate_table(codec, *inds, e16, e8, CANDS, per_image=per_image, pixels=px)
    assert {tab.modes[i] for i in range(len(CANDS))} == set(range(7))
    nb = tab.nbytes
    for ci, (c, m) in enumerate(CANDS):
        want, _, _ = _chain(codec, inds, e16, e8, c, m, per_image, px)
        assert torch.equal(nb[ci], want), (ci, nb[ci].cpu(), want.cpu())
    assert torch.equal(vq.usage_counter, counter) and int(vq.usage_hist.abs().sum()) == 0
    # the op form
    nb2 = torch.ops.cgic.rate_table(*inds, e16, e8, [c for c, _ in CANDS], [m for _, m in CANDS], per_image,
                                    codec.huffman.table.handle.value, px)
    assert torch.equal(nb, nb2)


def test_gathered_indices_equal_vq_of_merged_latent():
    rng = np.random.default_rng(5)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    qc = _conv(rng.standard_normal((4, 4)).astype(np.float32), rng.standard_normal(4).astype(np.float32))
    heads, e16, e8, px = _case(4, 128, 192, 3, "f32")
    inds = cg.grain_indices(vq, *heads, quant_conv=qc)
    for c, m in CANDS:
        masks, _, _, _ = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(e16, e8, want_gate=False, pixels=px)
        h = cg.grain_merge(*heads, masks)
        with torch.no_grad():
            want = cg.quantize._vq_forward(h, vq.embedding.weight, 0.25, True, None, False, False, quant_conv=qc)[2]
        got = torch.ops.cgic.gather_grain_indices(*inds, *masks)
        assert torch.equal(got.reshape(-1), want)


@pytest.mark.parametrize("fam_name", ["smooth8", "flat_edges", "blocky8"])
def test_rate_table_against_oracle(fam_name):
    B, H, W = 2, 256, 256
    x = families(n=B, H=H, W=W, seed=21)[fam_name]
    rng = np.random.default_rng(21)
    cb = rng.standard_normal((1024, 4)).astype(np.float32)
    heads = [rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32) for s in (16, 8, 4)]
    vq = _vq(cb)
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    e8, e16 = cg.entropy_maps(torch.from_numpy(x).to(DEV))
    inds = cg.grain_indices(vq, *[torch.from_numpy(h).to(DEV) for h in heads])
    tab = cg.rate_table(codec, *inds, e16.detach().clone(), e8.detach().clone(), CANDS, per_image=True)   # maps as given
    oind = [orc.vq(h, cb)[2].reshape(B, h.shape[2], h.shape[3]) for h in heads]
    htab = orc.HuffmanTable(FREQ)
    e16n, e8n = e16.cpu().numpy(), e8.cpu().numpy()
    nb = tab.nbytes.cpu().numpy()
    for ci, (c, m) in enumerate(CANDS):
        omc, omm, omf, _, mode = orc.router(e16n, e8n, c, m, per_image=True)
        for b in range(B):
            mc, mm, mf = omc[b, 0], omm[b, 0], omf[b, 0]
            up = lambda a, k: np.repeat(np.repeat(a, k, 0), k, 1)
            ind = np.where(mf == 1, oind[2][b], np.where(up(mm, 2) == 1, up(oind[1][b], 2), up(oind[0][b], 4)))
            streams = orc.compress_image(ind, mc, mm, mf, mode, htab)
            want = [len(streams[n]) if n in streams else 0 for n in orc.STREAM_NAMES]
            assert list(nb[ci, b]) == want, (fam_name, ci, b)


# ---- compress_to_bpp on a stand-in model -------------------------------------------------------------------------------------
class _Encoder(nn.Module):
    def __init__(self, c, m):
        super().__init__()
        self.conv_out_coarse = nn.Conv2d(3, 4, 16, stride=16)
        self.conv_out = nn.Conv2d(3, 4, 8, stride=8)
        self.conv_out_fine = nn.Conv2d(3, 4, 4, stride=4)
        self.router_config = {"target": "oracle.none", "params": {"coarse_grain_ratio": c, "medium_grain_ratio": m}}

    def forward(self, x, e16, e8):
        hc, hm, hf = self.conv_out_coarse(x), self.conv_out(x), self.conv_out_fine(x)
        mod, cls = self.router_config["target"].rsplit(".", 1)
        router = getattr(importlib.import_module(mod), cls)(**self.router_config["params"])
        mask, gate, fine_ratio, mode = router(e16, e8)
        h = cg.grain_merge(hc, hm, hf, mask)
        return {"h": h, "indices": None, "mask": mask, "fine_ratio": fine_ratio, "compression_mode": mode}


class _Decoder(nn.Module):
    def forward(self, quant2, quant, mask):
        return quant2 + 0.0 * quant


class _Model(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.encoder = _Encoder(0.1, 0.4)
        self.entropy_calculation_p8, self.entropy_calculation_p16 = cg.Entropy(8), cg.Entropy(16)
        self.quant_conv, self.post_quant_conv = nn.Conv2d(4, 4, 1), nn.Conv2d(4, 4, 1)
        self.quantize = cg.VectorQuantizer(1024, 4, beta=0.25)
        self.decoder = _Decoder()

    def encode(self, x):
        e8, e16 = self.entropy_calculation_p8(x), self.entropy_calculation_p16(x)
        d = self.encoder(x, e16, e8)
        quant, loss, ind = self.quantize(self.quant_conv(d["h"]))
        return quant, loss, d["indices"], d["mask"], ind, d["fine_ratio"], d["compression_mode"]

    def decode(self, quant, mask):
        return self.decoder(self.post_quant_conv(quant), quant, mask)


def _model():
    m = _Model().to(DEV).eval()
    with torch.no_grad():
        m.quantize.embedding.weight.normal_()
        m.quantize.usage_counter.copy_(torch.from_numpy(FREQ.astype(np.float32)))
    return cg.install(m)


def test_compress_to_bpp_matches_compress_batch():
    model = _model()
    x = torch.from_numpy(families(n=3, seed=4)["smooth8"]).to(DEV)
    counter = model.quantize.usage_counter.clone()
    cands = cg.default_candidates(0.1, 8) + [(0.0, 0.0), (1.0, 0.0)]
    with torch.no_grad():
        _, _, _, _, full = model.compress_to_bpp(x, 1e9, candidates=cands, decode=False)
    bb = full.batch_bpp.tolist()
    target = sorted(bb)[len(bb) // 2] + 1e-9
    with torch.no_grad():
        dec, bpp, comp, (c, m), tab = model.compress_to_bpp(x, target, candidates=cands)
    assert tab.fits
    best = max(v for v in bb if v <= target)
    assert tab.batch_bpp[cands.index((c, m))].item() == best
    params = model.encoder.router_config["params"]
    params["coarse_grain_ratio"], params["medium_grain_ratio"] = c, m
    with torch.no_grad():
        dec2, bpp2, comp2 = model.compress_batch(x)
    assert bpp == bpp2 and comp.to_host() == comp2.to_host() and torch.equal(dec, dec2)
    i1, _, _, _ = model._cgic_codec.decompress(comp, want_zq=False)
    i2, _, _, _ = model._cgic_codec.decompress(comp2, want_zq=False)
    assert torch.equal(i1, i2)
    assert [round(v, 12) for v in bpp] == [round(v, 12) for v in tab.bpp[cands.index((c, m))].tolist()]
    with torch.no_grad():
        _, _, _, _, low = model.compress_to_bpp(x, 1e-6, candidates=cands, decode=False)
    assert not low.fits
    assert torch.equal(model.quantize.usage_counter, counter)


def test_invalid_candidate_writes_nothing():
    rng = np.random.default_rng(9)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    heads, e16, e8, px = _case(2, 64, 64, 2, "f32")
    inds = cg.grain_indices(vq, *heads)
    C = 3
    cr = ctypes.c_double * C
    nbytes = torch.full((C, 2, 5), -777, dtype=torch.int32, device=DEV)
    B, h16, w16 = e16.shape
    ws = torch.full((_lib.lib().cgic_rate_table_workspace_bytes(B, h16, w16, C, 1),), 0xAB, dtype=torch.uint8, device=DEV)
    ws0 = ws.clone()
    pxa, keep = _lib.pixels_arg(px, B, h16, w16, 1)
    rc = _lib.lib().cgic_rate_table(codec.huffman.table.handle, _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]),
                                    _lib.ptr(e16), _lib.ptr(e8), B, h16, w16, C, cr(0.1, 0.5, 0.2), cr(0.8, 0.7, 0.1), 1, pxa,
                                    _lib.ptr(nbytes), _lib.ptr(ws), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID                      # (0.5, 0.7): fine < 0 -> k_medium > n
    assert int((nbytes != -777).sum()) == 0 and torch.equal(ws, ws0)
    with pytest.raises(cg.CgicError):
        cg.rate_table(codec, *inds, e16, e8, [(0.1, 0.5), (0.6, 0.6)])
