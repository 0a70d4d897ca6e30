"""GPU: the exact rate curve over every medium rank (cgic_rate_curve) and compress_to_bpp(search="curve") -- against the CPU
oracle at every rank a ratio reaches, against the real reference's file sizes (tests/golden/rate.npz), against the library's
own rate table, and end to end on the stand-in model of test_rate_control.py."""
import os

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib
from oracle import cgic_oracle as orc
from oracle.content_families import families

from test_rate_control import FREQ, _conv, _model, _vq

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))


def _up(a, k):
    return np.repeat(np.repeat(a, k, 0), k, 1)


def _oracle_sizes(e16n, e8n, oind, htab, c, m):
    """[B][5]: the oracle's router on the maps -> the per-head indices gathered through its masks -> the oracle's coder"""
    omc, omm, omf, _, mode = orc.router(e16n, e8n, c, m, per_image=True)
    out = []
    for b in range(e16n.shape[0]):
        mc, mm, mf = omc[b, 0], omm[b, 0], omf[b, 0]
        ind = np.where(mf == 1, oind[2][b], np.where(_up(mm, 2) == 1, _up(oind[1][b], 2), _up(oind[0][b], 4)))
        streams = orc.compress_image(ind, mc, mm, mf, mode, htab)
        out.append([len(streams[n]) if n in streams else 0 for n in orc.STREAM_NAMES])
    return out, omc


@pytest.mark.parametrize("coarse", [0.1, 0.3, 0.0])
@pytest.mark.parametrize("fam_name", ["noise8", "smooth8", "flat_edges", "blocky8"])
def test_rate_curve_against_oracle_every_rank(fam_name, coarse):
    B, H, W = 2, 256, 256
    x = families(n=B, H=H, W=W, seed=21)[fam_name]
    rng = np.random.default_rng(21)
    cb = rng.standard_normal((1024, 4)).astype(np.float32)
    heads = [rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32) for s in (16, 8, 4)]
    vq = _vq(cb)
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    e8, e16 = cg.entropy_maps(torch.from_numpy(x).to(DEV), reference_order=True)
    inds = cg.grain_indices(vq, *[torch.from_numpy(h).to(DEV) for h in heads])
    counter = vq.usage_counter.clone()
    curve = cg.rate_curve(codec, *inds, e16, e8, coarse)
    assert torch.equal(vq.usage_counter, counter)
    n16 = (H // 16) * (W // 16)
    n8 = 4 * n16
    assert tuple(curve.nbytes.shape) == (B, n8 + 1, 5) and curve.batch_bpp.shape == (n8 + 1,)
    # every rank a ratio reaches in the curve's mode: one run from round(4 n16 c) to n8
    assert curve.ranks == list(range(round(4 * n16 * coarse), n8 + 1))
    oind = [orc.vq(h, cb)[2].reshape(B, h.shape[2], h.shape[3]) for h in heads]
    htab = orc.HuffmanTable(FREQ)
    e16n, e8n = e16.cpu().numpy(), e8.cpu().numpy()
    nb = curve.nbytes.cpu().numpy()
    wrong = []
    for K, (c, m) in zip(curve.ranks, curve.candidates):
        assert c == coarse and cg.router_ranks(c, m, n16)[1] == K
        want, omc = _oracle_sizes(e16n, e8n, oind, htab, c, m)
        if nb[:, K].tolist() != want:
            wrong.append((K, m, nb[:, K].tolist(), want))
    assert not wrong, (fam_name, coarse, len(wrong), wrong[:3])
    assert curve.n_coarse.tolist() == [int(omc[b].sum()) for b in range(B)]
    assert torch.equal(curve.bytes, curve.nbytes.cpu().to(torch.int64).sum(dim=2))
    assert curve.bpp[1, n8].item() == int(nb[1, n8].sum()) * 8 / (H * W)


def test_golden_reference_sizes_on_the_curve():
    """the real reference's file sizes: the mode 0 / mode 1 candidates of rate.npz are ranks of the curve of their coarse ratio"""
    g = np.load(os.path.join(HERE, "golden", "rate.npz"))
    cand = [tuple(float(v) for v in r) for r in g["candidates"]]
    vq = _vq(g["codebook"])
    qc = _conv(g["qc_w"], g["qc_b"])
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    checked = 0
    for ii in range(len(g["names"])):
        x = torch.from_numpy(g[f"img{ii}_x"].transpose(2, 0, 1)[None].astype(np.float32) / 255.0).to(DEV)
        e8, e16 = cg.entropy_maps(x, reference_order=True)
        heads = [torch.from_numpy(g[f"img{ii}_h{k}"]).to(DEV) for k in "cmf"]
        inds = cg.grain_indices(vq, *heads, quant_conv=qc)
        curves = {}
        for ci, (c, m) in enumerate(cand):
            mode = int(g[f"img{ii}_c{ci}_mode"])
            if mode not in (0, 1):
                continue
            if c not in curves:
                curves[c] = cg.rate_curve(codec, *inds, e16, e8, c)
            curve = curves[c]
            K = cg.router_ranks(c, m, 256)[1]
            assert K in curve.ranks and curve.modes[curve.ranks.index(K)] == mode
            sizes = g[f"img{ii}_c{ci}_sizes"]
            got = curve.nbytes[0, K].cpu().numpy()
            assert np.array_equal(got, sizes), (ii, ci, K, got, sizes)
            assert curve.bpp[0, K].item() == sizes.sum() * 8 / (256 * 256)
            checked += 1
    assert checked == 2 * sum(orc.router_mode(c, m) in (0, 1) for c, m in cand) and checked >= 8


@pytest.mark.parametrize("B,H,W", [(64, 256, 256), (1, 768, 768), (3, 64, 96)])
@pytest.mark.parametrize("coarse", [0.1, 0.0])
def test_rate_curve_equals_rate_table_at_sampled_ranks(B, H, W, coarse):
    rng = np.random.default_rng(B + H)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    fam = families(n=B, H=H, W=W, seed=B + W)
    x = torch.from_numpy(fam["smooth8" if B > 1 else "flat_edges"]).to(DEV)
    heads = [torch.from_numpy(rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32)).to(DEV) for s in (16, 8, 4)]
    e8, e16 = cg.entropy_maps(x)
    e16, e8 = e16.detach().clone(), e8.detach().clone()                 # maps as given: no pixels behind them
    inds = cg.grain_indices(vq, *heads)
    curve = cg.rate_curve(codec, *inds, e16, e8, coarse)
    assert len(curve.ranks) >= 64
    pick = sorted({curve.ranks[i] for i in np.linspace(0, len(curve.ranks) - 1, 64).round().astype(int)})
    cands = [curve.ratio(K) for K in pick]
    tab = cg.rate_table(codec, *inds, e16, e8, cands, per_image=True)
    assert set(tab.modes) == {0 if coarse > 0 else 1}
    want = tab.nbytes.permute(1, 0, 2)                                   # [B, C, 5]
    got = curve.nbytes[:, torch.tensor(pick, device=DEV)]
    assert torch.equal(got, want), (got != want).nonzero()[:5].tolist()
    # the op form
    nb2 = torch.ops.cgic.rate_curve(*inds, e16, e8, coarse, codec.huffman.table.handle.value)
    assert torch.equal(nb2, curve.nbytes)


def test_compress_to_bpp_curve_search():
    model = _model()
    x = torch.from_numpy(families(n=3, seed=4)["smooth8"]).to(DEV)
    counter = model.quantize.usage_counter.clone()
    params = model.encoder.router_config["params"]
    c0, m0 = params["coarse_grain_ratio"], params["medium_grain_ratio"]
    with torch.no_grad():
        _, _, _, _, full = model.compress_to_bpp(x, 1e9, decode=False, search="curve")
        _, _, _, _, tab = model.compress_to_bpp(x, 1e9, decode=False)
    assert isinstance(full, cg.RateCurve) and isinstance(tab, cg.RateTable) and len(full.ranks) > 900
    lo, hi = float(tab.batch_bpp.min()), float(tab.batch_bpp.max())
    for frac in (0.25, 0.5, 0.75):
        target = lo + frac * (hi - lo)
        with torch.no_grad():
            dec, bpp, comp, (c, m), curve = model.compress_to_bpp(x, target, search="curve")
            dec_t, bpp_t, comp_t, (ct, mt), tab_t = model.compress_to_bpp(x, target)
        got, got_t = sum(bpp) / len(bpp), sum(bpp_t) / len(bpp_t)
        print(f"target {target:.6f} bpp: curve {got:.6f} ({target - got:.6f} under, rank {curve.chosen_rank}), "
              f"16 candidates {got_t:.6f} ({target - got_t:.6f} under)")
        assert curve.fits and tab_t.fits and c == c0
        assert got_t <= got <= target
        # its bpp is the curve's entry of the chosen rank (or of the chosen end)
        if curve.chosen_rank is not None:
            assert cg.router_ranks(c, m, 256)[1] == curve.chosen_rank
            assert bpp == curve.bpp[:, curve.chosen_rank].tolist()
        else:
            assert bpp == curve.ends.bpp[curve.ends.candidates.index((c, m))].tolist()
        best = max(v for v in curve.batch_bpp[torch.tensor(curve.ranks)].tolist() + curve.ends.batch_bpp.tolist() if v <= target)
        assert abs(got - best) < 1e-12
        # bit-identical to compress_batch at the returned ratio
        params["coarse_grain_ratio"], params["medium_grain_ratio"] = c, m
        try:
            with torch.no_grad():
                dec2, bpp2, comp2 = model.compress_batch(x)
        finally:
            params["coarse_grain_ratio"], params["medium_grain_ratio"] = c0, m0
        assert bpp == bpp2 and comp.to_host() == comp2.to_host() and torch.equal(dec, dec2)
        # search="candidates" is what compress_to_bpp was: the default candidates, the table's choice
        cands = cg.default_candidates(c0)
        i, fits = cg.choose(tab_t, target)
        assert tab_t.candidates == cands and (ct, mt) == cands[i] and fits
        with torch.no_grad():
            _, bpp_e, comp_e, r_e, _ = model.compress_to_bpp(x, target, candidates=cands, search="candidates")
        assert r_e == (ct, mt) and bpp_e == bpp_t and comp_e.to_host() == comp_t.to_host()
    with torch.no_grad():
        _, _, _, _, low = model.compress_to_bpp(x, 1e-6, decode=False, search="curve")
    assert not low.fits
    assert torch.equal(model.quantize.usage_counter, counter) and int(model.quantize.usage_hist.abs().sum()) == 0
    with pytest.raises(ValueError):
        model.compress_to_bpp(x, 0.5, search="bisect")
    with pytest.raises(ValueError):
        model.compress_to_bpp(x, 0.5, candidates=[(0.1, 0.4)], search="curve")


def test_symbol_outside_the_table_is_a_key_error():
    rng = np.random.default_rng(9)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    B, H, W = 2, 64, 64
    x = torch.from_numpy(families(n=B, H=H, W=W, seed=2)["smooth8"]).to(DEV)
    heads = [torch.from_numpy(rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32)).to(DEV) for s in (16, 8, 4)]
    e8, e16 = cg.entropy_maps(x, reference_order=True)
    inds = [t.clone() for t in cg.grain_indices(vq, *heads)]
    good = torch.ops.cgic.rate_curve(*inds, e16, e8, 0.1, codec.huffman.table.handle.value).cpu()
    assert int(good.min()) >= 0
    n16, n8 = 16, 64
    k_c = cg.router_ranks(0.1, 0.4, n16)[0]
    assert k_c == 2

    def noncoarse_e8(b, fill):
        thr = e16[b].flatten().sort().values[k_c - 1]
        nc = (~(e16[b] < thr)).repeat_interleave(2, 0).repeat_interleave(2, 1)
        return torch.where(nc, e8[b], torch.full_like(e8[b], fill))

    # image 1: a MEDIUM symbol outside the table at the non-coarse patch of the lowest entropy -- selected at every rank that
    # selects a medium patch at all.  image 0: a FINE symbol outside the table inside the non-coarse patch of the highest
    # entropy -- selected at every rank that leaves a fine patch at all
    p = int(noncoarse_e8(1, float("inf")).argmin())
    inds[1].view(B, -1)[1, p] = 1024
    q = int(noncoarse_e8(0, -1.0).argmax())
    inds[2].view(B, 16, 16)[0, 2 * (q // 8) + 1, 2 * (q % 8)] = -3
    ws = torch.empty(_lib.lib().cgic_rate_curve_workspace_bytes(B, 4, 4), dtype=torch.uint8, device=DEV)
    nb = torch.empty((B, n8 + 1, 5), dtype=torch.int32, device=DEV)
    _lib.call("cgic_rate_curve", codec.huffman.table.handle, _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]), _lib.ptr(e16),
              _lib.ptr(e8), B, 4, 4, 0.1, _lib.ptr(nb), _lib.ptr(ws), _lib.current_stream())
    nb = nb.cpu()
    neg = nb < 0
    assert set(nb[neg].tolist()) == {_lib.ERR_INVALID - 10}
    assert torch.equal(nb[~neg], good[~neg])
    for b, s in ((1, 1), (0, 2)):
        other = [i for i in range(5) if i != s]
        assert int(neg[b][:, other].sum()) == 0
        assert torch.equal(neg[b][:, s], good[b][:, s] > 0) and int(neg[b][:, s].sum()) > 0
    with pytest.raises(KeyError):
        cg.rate_curve(codec, *inds, e16, e8, 0.1)
    with pytest.raises(KeyError):                                                  # as RateTable
        cg.rate_table(codec, *inds, e16, e8, [(0.1, 0.4)], per_image=True)
