"""GPU: the device-side rate pick (cgic_route_to_budget, route_to_bpp, compress_to_bpp(search="device")) -- against the
project's own host path (rate_curve -> choose -> router -> gather_grain_indices -> compress) at targets taken from the host
curve, against the CPU oracle's router on the small shapes, inside a captured graph, and end to end on the stand-in model of
test_rate_control.py."""
import functools
import math

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, rate
from oracle import cgic_oracle as orc
from oracle.content_families import families

from test_rate_control import FREQ, _model, _vq

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(2, 64, 64), (3, 64, 96), (64, 256, 256), (1, 768, 768)]


@functools.lru_cache(maxsize=None)
def _codec(uniform=False):
    rng = np.random.default_rng(31)
    vq = _vq(rng.standard_normal((1024, 4)).astype(np.float32))
    if uniform:                                                        # every code 10 bits long
        vq.usage_counter.fill_(1.0)
    return vq, cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)


@functools.lru_cache(maxsize=None)
def _content(B, H, W):
    return families(n=B, H=H, W=W, seed=B + W)


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W, fam_name, uniform=False):
    """(inds, e16, e8) of one case, made once: the maps as given (no pixels behind them: routing does not refine)"""
    vq, _ = _codec(uniform)
    rng = np.random.default_rng(B + H)
    heads = [torch.from_numpy(rng.standard_normal((B, 4, H // s, W // s)).astype(np.float32)).to(DEV) for s in (16, 8, 4)]
    inds = cg.grain_indices(vq, *heads)
    e8, e16 = cg.entropy_maps(torch.from_numpy(_content(B, H, W)[fam_name]).to(DEV), reference_order=True)
    return inds, e16.detach().clone(), e8.detach().clone()


def _host_curve(codec, inds, e16, e8, coarse):
    K, m = rate.reachable_ranks_vec(e16.shape[1] * e16.shape[2], float(coarse))
    return cg.rate_curve(codec, *inds, e16, e8, coarse, ranks=tuple(zip(K.tolist(), m.tolist())))


def _host_route(codec, inds, e16, e8, curve, K):
    c, m = curve.ratio(K)
    masks, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(e16, e8, want_gate=False)
    ind = cg.gather_grain_indices(*inds, masks)
    return masks, ind, mode, (c, m)


def _targets(curve):
    bb = curve.batch_bpp[torch.tensor(curve.ranks, dtype=torch.int64)]
    out = []
    for frac in (0.25, 0.5, 0.75):
        t = curve.batch_bpp[curve.ranks[int(frac * (len(curve.ranks) - 1))]].item()
        out += [t, math.nextafter(t, -math.inf)]
    return out + [math.nextafter(float(bb.min()), -math.inf), float(bb.max()) + 1.0]


def _assert_route_is_host(codec, inds, e16, e8, curve, route, target, host_cache, oracle=False):
    K, fits = cg.choose(curve, target)
    assert (route.rank, route.fits) == (K, fits), (target, route.rank, route.fits, K, fits)
    assert route.batch_bytes == int(curve.bytes[:, K].sum())
    assert route.ratio == curve.ratio(K)
    if K not in host_cache:
        masks, ind, mode, (c, m) = _host_route(codec, inds, e16, e8, curve, K)
        host_cache[K] = (masks, ind, mode, codec.compress(ind, masks, mode).to_host(), (c, m))
    masks, ind, mode, streams, (c, m) = host_cache[K]
    assert route.mode == mode == (0 if curve.coarse_ratio > 0 else 1)
    for got, want in zip(route.masks, masks):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    assert route.ind.shape == ind.shape and torch.equal(route.ind, ind)
    assert codec.compress(route.ind, route.masks, route.mode).to_host() == streams
    if oracle:
        om = orc.router(e16.cpu().numpy(), e8.cpu().numpy(), c, m, per_image=True)
        assert om[4] == mode
        for got, want in zip(route.masks, om[:3]):
            assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
    return K


@pytest.mark.parametrize("coarse", [0.1, 0.3, 0.0])
@pytest.mark.parametrize("fam_name", ["smooth8", "flat_edges", "noise8"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_pick_and_masks_equal_the_host_path(B, H, W, fam_name, coarse):
    _, codec = _codec()
    inds, e16, e8 = _inputs(B, H, W, fam_name)
    curve = _host_curve(codec, inds, e16, e8, coarse)
    host_cache, seen_fits = {}, set()
    for target in _targets(curve):
        route = cg.route_to_bpp(codec, *inds, e16, e8, coarse, target_bpp=target)
        _assert_route_is_host(codec, inds, e16, e8, curve, route, target, host_cache, oracle=H == 64)
        seen_fits.add(route.fits)
    assert seen_fits == {True, False} and len(host_cache) >= 2


def test_tie_break_takes_the_smaller_rank():
    """equal batch sizes at two ranks: with every code 10 bits long a size changes only when a patch changes its grain, and the
    ranks inside a group of tied entropies (flat_edges: zero and tied patches) select the same patches"""
    _, codec = _codec(uniform=True)
    B, H, W, coarse = 2, 64, 64, 0.1
    inds, e16, e8 = _inputs(B, H, W, "flat_edges", uniform=True)
    curve = _host_curve(codec, inds, e16, e8, coarse)
    S = curve.bytes.sum(dim=0)
    tied = [(a, b) for a, b in zip(curve.ranks, curve.ranks[1:]) if int(S[a]) == int(S[b])]
    if not tied:
        pytest.skip("no two reachable ranks of this content have the same batch size")
    host_cache = {}
    top = max(int(S[k]) for k in curve.ranks)
    for a, b in (tied[0], tied[-1]):
        target = curve.batch_bpp[a].item()
        route = cg.route_to_bpp(codec, *inds, e16, e8, coarse, target_bpp=target)
        K = _assert_route_is_host(codec, inds, e16, e8, curve, route, target, host_cache)
        first = min(k for k in curve.ranks if int(S[k]) == int(S[a]))
        assert K == first and K <= a < b and route.batch_bytes == int(S[b])
    # the same rule without a fit: the smallest size, the smaller rank
    low = min(int(S[k]) for k in curve.ranks)
    route = cg.route_to_bpp(codec, *inds, e16, e8, coarse, target_bpp=0.0)
    assert not route.fits and route.rank == min(k for k in curve.ranks if int(S[k]) == low) and top >= low
    _assert_route_is_host(codec, inds, e16, e8, curve, route, 0.0, host_cache)


def test_symbol_outside_the_table_is_a_key_error():
    vq, codec = _codec()
    B, H, W = 2, 64, 64
    good, e16, e8 = _inputs(B, H, W, "smooth8")
    inds = [t.clone() for t in good]
    k_c = cg.router_ranks(0.1, 0.4, 16)[0]
    assert k_c == 2

    def noncoarse_e8(b, fill):
        thr = e16[b].flatten().sort().values[k_c - 1]
        nc = (~(e16[b] < thr)).repeat_interleave(2, 0).repeat_interleave(2, 1)
        return torch.where(nc, e8[b], torch.full_like(e8[b], fill))

    # (the planted indices of test_rate_curve.py: a medium symbol outside the table at the non-coarse patch of the lowest
    # entropy of image 1, a fine one inside the non-coarse patch of the highest entropy of image 0)
    p = int(noncoarse_e8(1, float("inf")).argmin())
    inds[1].view(B, -1)[1, p] = 1024
    q = int(noncoarse_e8(0, -1.0).argmax())
    inds[2].view(B, 16, 16)[0, 2 * (q // 8) + 1, 2 * (q % 8)] = -3
    with pytest.raises(KeyError):
        cg.rate_curve(codec, *inds, e16, e8, 0.1)
    route = cg.route_to_bpp(codec, *inds, e16, e8, 0.1, target_bpp=1.0)
    assert route.choice.cpu().tolist() == [-1, -1, 0, -1]
    for name in ("rank", "ratio", "fits", "batch_bytes"):
        with pytest.raises(KeyError):
            getattr(route, name)
    for t in route.masks + [route.ind]:
        assert int(t.abs().max()) == 0
    # the next ordinary call on the same codec
    curve = _host_curve(codec, good, e16, e8, 0.1)
    route = cg.route_to_bpp(codec, *good, e16, e8, 0.1, target_bpp=1.0)
    _assert_route_is_host(codec, good, e16, e8, curve, route, 1.0, {})


def test_graph_capture_and_replay_with_new_budgets():
    _, codec = _codec()
    B, H, W, coarse = 2, 64, 64, 0.1
    inds, e16, e8 = _inputs(B, H, W, "smooth8")
    curve = _host_curve(codec, inds, e16, e8, coarse)
    budget = torch.zeros(1, dtype=torch.int64, device=DEV)
    cg.route_to_bpp(codec, *inds, e16, e8, coarse, budget=budget)       # (the rank list and the code table are uploaded once)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # a synchronising call in here raises
        route = cg.route_to_bpp(codec, *inds, e16, e8, coarse, budget=budget)
    targets = _targets(curve)
    picked = set()
    for target in (targets[0], targets[5], targets[6]):
        bud = cg.budget_bytes(target, H * W, B)
        budget.copy_(torch.tensor([bud], dtype=torch.int64))
        g.replay()
        route.refresh()
        eager = cg.route_to_bpp(codec, *inds, e16, e8, coarse, budget=torch.tensor([bud], dtype=torch.int64, device=DEV))
        assert route.choice.tolist() == eager.choice.tolist()
        for got, want in zip(route.masks + [route.ind], eager.masks + [eager.ind]):
            assert torch.equal(got, want)
        picked.add(_assert_route_is_host(codec, inds, e16, e8, curve, route, target, {}))
    assert len(picked) == 3
    with pytest.raises(ValueError):
        cg.route_to_bpp(codec, *inds, e16, e8, coarse)
    with pytest.raises(ValueError):
        cg.route_to_bpp(codec, *inds, e16, e8, coarse, target_bpp=1.0, budget=budget)
    with pytest.raises(ValueError):
        cg.route_to_bpp(codec, *inds, e16, e8, coarse, budget=budget.to(torch.int32))


def test_compress_to_bpp_device_search():
    model = _model()
    x = torch.from_numpy(families(n=3, seed=4)["smooth8"]).to(DEV)
    counter = model.quantize.usage_counter.clone()
    params = model.encoder.router_config["params"]
    c0, m0 = params["coarse_grain_ratio"], params["medium_grain_ratio"]
    with torch.no_grad():
        _, _, _, _, full = model.compress_to_bpp(x, 1e9, decode=False, search="curve")
    for frac in (0.25, 0.5, 0.75):
        target = full.batch_bpp[full.ranks[int(frac * (len(full.ranks) - 1))]].item()
        with torch.no_grad():
            dec, bpp, comp, (c, m), route = model.compress_to_bpp(x, target, search="device")
            dec_h, bpp_h, comp_h, (ch, mh), curve = model.compress_to_bpp(x, target, search="curve")
        assert isinstance(route, cg.BppRoute)
        assert curve.chosen_rank is not None
        assert (route.rank, route.fits, (c, m)) == (curve.chosen_rank, curve.fits, (ch, mh)) and route.ratio == (c, m)
        assert route.batch_bytes == int(curve.bytes[:, curve.chosen_rank].sum())
        assert bpp == bpp_h == curve.bpp[:, curve.chosen_rank].tolist()
        assert comp.to_host() == comp_h.to_host() and torch.equal(dec, dec_h)
        # bit-identical to compress_batch at the returned ratio
        params["coarse_grain_ratio"], params["medium_grain_ratio"] = c, m
        try:
            with torch.no_grad():
                dec2, bpp2, comp2 = model.compress_batch(x)
        finally:
            params["coarse_grain_ratio"], params["medium_grain_ratio"] = c0, m0
        assert bpp == bpp2 and comp.to_host() == comp2.to_host() and torch.equal(dec, dec2)
    with torch.no_grad():
        dec, _, _, _, low = model.compress_to_bpp(x, 1e-6, decode=False, search="device")
    assert dec is None and not low.fits
    assert torch.equal(model.quantize.usage_counter, counter) and int(model.quantize.usage_hist.abs().sum()) == 0
    with pytest.raises(ValueError):
        model.compress_to_bpp(x, 0.5, search="bisect")
    with pytest.raises(ValueError):
        model.compress_to_bpp(x, 0.5, candidates=[(0.1, 0.4)], search="device")


@pytest.mark.parametrize("coarse", [0.1, 0.0])
def test_op_form_equals_the_function(coarse):
    _, codec = _codec()
    B, H, W = 3, 64, 96
    inds, e16, e8 = _inputs(B, H, W, "smooth8")
    budget = torch.tensor([cg.budget_bytes(2.0, H * W, B)], dtype=torch.int64, device=DEV)
    route = cg.route_to_bpp(codec, *inds, e16, e8, coarse, budget=budget)
    mc, mm, mf, ind, choice = torch.ops.cgic.route_to_bpp(*inds, e16, e8, coarse, budget, codec.huffman.table.handle.value)
    assert route.rank >= 0
    assert choice.tolist() == route.choice.tolist()
    for got, want in zip((mc, mm, mf, ind), route.masks + [route.ind]):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def test_rate_curve_op_still_equals_the_entry_point():
    """nothing changed: the curve's op against cgic_rate_curve through ctypes (the three curve kernels share one body)"""
    _, codec = _codec()
    B, H, W = 2, 64, 64
    inds, e16, e8 = _inputs(B, H, W, "flat_edges")
    n8 = 64
    ws = torch.empty(_lib.lib().cgic_rate_curve_workspace_bytes(B, 4, 4), dtype=torch.uint8, device=DEV)
    nb = torch.empty((B, n8 + 1, 5), dtype=torch.int32, device=DEV)
    _lib.call("cgic_rate_curve", codec.huffman.table.handle, _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]), _lib.ptr(e16),
              _lib.ptr(e8), B, 4, 4, 0.1, _lib.ptr(nb), _lib.ptr(ws), _lib.current_stream())
    op = torch.ops.cgic.rate_curve(*inds, e16, e8, 0.1, codec.huffman.table.handle.value)
    assert torch.equal(op, nb) and int(nb.min()) >= 0 and int(nb.sum()) > 0
