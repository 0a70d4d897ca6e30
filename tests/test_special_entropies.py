"""GPU: the router and every rate-control entry point on entropy maps that hold NaN, +-Inf, negatives, signed zeros and denormals.

The library makes such maps itself (a NaN pixel is a NaN 8x8 and a NaN 16x16 entropy, like the reference's histogram) and every
rate call takes its maps as given.  The checkers: the real router's masks (tests/golden/router_specials.npz), the CPU oracle's
router (pinned to them by tests/test_oracle_golden.py) and the plain numpy reference at explicit ranks of tests/specials_ref.py
(pinned to the oracle by tests/test_specials_host.py).  Every comparison is exact.
"""
import functools

import numpy as np
import pytest
import torch

import control_gic_amd as cg
import specials_ref as sr
from control_gic_amd import _lib, rate
from oracle import cgic_oracle as orc
from oracle.content_families import families

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = len(sr.SHAPES)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(t, a):
    """a device float32 tensor holds exactly these bits (the upload did not touch a NaN payload, a zero's sign or a denormal)"""
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.asarray(a, np.float32).view(np.uint32))


def _masks_equal(got, want):
    return [int((g.cpu().numpy().reshape(w.shape) != w).sum()) for g, w in zip(got, want)]


@functools.lru_cache(maxsize=None)
def _zipf():
    """(GrainCodec on the 1024-symbol Zipf table, the oracle's code lengths of the same table)"""
    rng = np.random.default_rng(31)
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    vq.embedding.weight.data.copy_(torch.from_numpy(rng.standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(sr.FREQ.astype(np.float32)))
    codec = cg.GrainCodec(cg.HuffmanCoding(vq.embedding_counter), vq.embedding.weight)
    lens = orc.HuffmanTable(sr.FREQ).len
    assert codec.huffman.table.arrays()[0] == lens.tolist()
    return vq, codec, lens


@functools.lru_cache(maxsize=None)
def _big_table():
    """(HuffmanCoding of 4096 symbols, the oracle's code lengths): 16 KB of code lengths, more than the 8 KB a 48x64 curve has left"""
    n = 4096
    freq = np.floor(1e7 / (1 + np.arange(n)) ** 1.05).astype(np.int64) + 1
    coder = cg.HuffmanCoding({str(int(k)): torch.tensor([float(freq[int(k)])]) for k in orc.param_dict_order(n)})
    lens = orc.HuffmanTable(freq).len
    assert coder.table.arrays()[0] == lens.tolist() and int(lens.max()) <= 4095
    return coder, lens


@functools.lru_cache(maxsize=None)
def _heads_indices(B, h16, w16, seed, nsym=1024):
    """grain indices [B, h, w] x 3 (device int64, host numpy): of finite random heads through the Zipf codebook, or -- for a table
    that has no codebook -- seeded indices"""
    rng = np.random.default_rng(seed)
    if nsym == 1024:
        vq = _zipf()[0]
        heads = [_t(rng.standard_normal((B, 4, s * h16, s * w16)).astype(np.float32)) for s in (1, 2, 4)]
        inds = tuple(cg.grain_indices(vq, *heads))
    else:
        inds = tuple(_t(rng.integers(0, nsym, (B, s * h16, s * w16)).astype(np.int64)) for s in (1, 2, 4))
    return inds, tuple(t.cpu().numpy() for t in inds)


def _fixture(golden, si, cls):
    g = golden("router_specials")
    return g[f"s{si}_{cls}_e16"], g[f"s{si}_{cls}_e8"]


# ---------------------------------------------------------------------------- the router, stand-alone and fused, on the fixture
@pytest.mark.parametrize("si", range(NS))
def test_router_equals_the_real_routers_masks(golden, si):
    """stage 1, one band (every fixture shape fits one workgroup's LDS): all classes, ratio pairs of all seven modes, the flattened
    batch and image by image"""
    g = golden("router_specials")
    for cls in sr.CLASSES:
        e16, e8 = _fixture(golden, si, cls)
        d16, d8 = _t(e16), _t(e8)
        assert _same_bits(d16, e16) and _same_bits(d8, e8)
        want = sr.fixture_masks(g, si, cls)
        for ri, (c, m) in enumerate(sr.RATIOS):
            for how in ("batch", "per"):
                mask, gate, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=how == "per")(d16, d8)
                assert mode == int(g[f"r{ri}_mode"])
                assert _masks_equal(mask, want[(ri, how)]) == [0, 0, 0], (si, cls, c, m, how, _masks_equal(mask, want[(ri, how)]))
                assert np.array_equal(gate.cpu().numpy(), orc.router(e16, e8, c, m, per_image=how == "per")[3])


@pytest.mark.parametrize("si", [i for i, s in enumerate(sr.SHAPES) if s[0] >= 2])
def test_fused_vq_router_launch_equals_the_real_routers_masks(golden, si):
    from control_gic_amd.quantize import _vq_forward, vq_forward_route
    g = golden("router_specials")
    B, h16, w16 = sr.SHAPES[si]
    rng = np.random.default_rng(si)
    z = _t(rng.standard_normal((B, 4, 4 * h16, 4 * w16)).astype(np.float32))
    w = _t(rng.standard_normal((1024, 4)).astype(np.float32))
    zq0, loss0, idx0 = _vq_forward(z, w, 0.25, True, None)
    for cls in sr.CLASSES:
        e16, e8 = _fixture(golden, si, cls)
        d16, d8 = _t(e16), _t(e8)
        want = sr.fixture_masks(g, si, cls)
        for ri, (c, m) in enumerate(sr.RATIOS):
            for how in ("batch", "per"):
                for q in (False, True):
                    zq, loss, idx, mask, _, mode = vq_forward_route(z, w, 0.25, True, d16, d8, c, m, per_image=how == "per", refine_queues=q)
                    assert mode == int(g[f"r{ri}_mode"])
                    assert _masks_equal(mask, want[(ri, how)]) == [0, 0, 0], (si, cls, c, m, how, q)
        assert torch.equal(idx, idx0) and torch.equal(zq, zq0) and torch.equal(loss, loss0)


# ---------------------------------------------------------------------------- one seeded case per path of the router's plan
def _router_stage(N16, budget=96 * 1024):
    """router_lds_bytes (cgic_encode_plan.h) without refinement, for the stand-alone launch's 96 KB: the stage of a segment of N16
    coarse patches (tests/test_encode_plan_host.py runs the header itself on these shapes)"""
    lds = 4096 + 8 * ((N16 + 63) // 64)
    return 1 if lds + 20 * N16 <= budget else 2 if lds + 16 * N16 <= budget else 0


PLAN_RATIOS = [(0.1, 0.8), (0.3, 0.3), (0.0, 0.4), (0.4, 0.0), (0.3, 0.7)]


@pytest.mark.parametrize("cls", ["mix", "nan_pixels", "gated", "neg"])
def test_router_row_bands_of_a_768_tile(cls):
    """stage 1 with row bands: one 768x768 tile's maps (48x48 coarse patches), per image: 8 workgroups repeat the selects and write
    a band of rows each"""
    assert _router_stage(48 * 48) == 1                                   # (bands: 8, router_plan)
    e16, e8 = sr.special_maps(1, 48, 48, cls, seed=48, levels=24)
    d16, d8 = _t(e16), _t(e8)
    for c, m in PLAN_RATIOS:
        mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(d16, d8, want_gate=False)
        o = orc.router(e16, e8, c, m, per_image=True, want_gate=False)
        assert mode == o[4] and _masks_equal(mask, o[:3]) == [0, 0, 0], (cls, c, m, _masks_equal(mask, o[:3]))


@pytest.mark.parametrize("B,stage", [(20, 2), (32, 0), (48, 0)])
@pytest.mark.parametrize("cls", ["mix", "nan_pixels", "gated"])
def test_router_batch_global_segments_beyond_stage_one(cls, B, stage):
    """batch-global segments of B x 16x16 coarse patches, maps as given, no pixels: 5 120 patches stage only e8 (stage 2); 8 192 and
    12 288 stage nothing (stage 0)"""
    assert _router_stage(B * 256) == stage
    e16, e8 = sr.special_maps(B, 16, 16, cls, seed=B, levels=24)
    d16, d8 = _t(e16), _t(e8)
    for c, m in PLAN_RATIOS:
        mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=False)(d16, d8, want_gate=False)
        o = orc.router(e16, e8, c, m, per_image=False, want_gate=False)
        assert mode == o[4] and _masks_equal(mask, o[:3]) == [0, 0, 0], (cls, B, c, m, _masks_equal(mask, o[:3]))


# ---------------------------------------------------------------------------- from pixels: entropy_maps -> router with refinement
def _nan_pixels(x, seed):
    """a few NaN pixels per image: isolated ones and one whole 16x16 patch"""
    x = x.copy()
    rng = np.random.default_rng(seed)
    B, _, H, W = x.shape
    for b in range(B):
        for _ in range(3):
            x[b, rng.integers(0, 3), rng.integers(0, H), rng.integers(0, W)] = np.nan
        y, xx = 16 * int(rng.integers(0, H // 16)), 16 * int(rng.integers(0, W // 16))
        x[b, :, y:y + 16, xx:xx + 16] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def _pixel_case(name, B, H, W):
    x = _nan_pixels(families(n=B, H=H, W=W, seed=B + W)[name], seed=H)
    return x, orc.entropy_ref(x, 8), orc.entropy_ref(x, 16)


@pytest.mark.parametrize("B,H,W", [(3, 64, 96), (2, 256, 256)])
@pytest.mark.parametrize("name", ["flat_edges", "smooth8"])
def test_router_from_pixels_with_nan_pixels(name, B, H, W):
    from control_gic_amd.quantize import vq_forward_route
    x, a8, a16 = _pixel_case(name, B, H, W)
    assert np.isnan(a16).sum() >= B and np.isnan(a8).sum() >= 4 * B
    xd = _t(x)
    e8, e16 = cg.entropy_maps(xd)
    assert np.array_equal(np.isnan(e8.cpu().numpy()), np.isnan(a8)) and np.array_equal(np.isnan(e16.cpu().numpy()), np.isnan(a16))
    rng = np.random.default_rng(B)
    z = _t(rng.standard_normal((B, 4, H // 4, W // 4)).astype(np.float32))
    w = _t(rng.standard_normal((1024, 4)).astype(np.float32))
    for c, m in PLAN_RATIOS:
        o = orc.router(a16, a8, c, m, per_image=True, want_gate=False)
        mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(e16, e8, want_gate=False, pixels=xd)
        assert mode == o[4] and _masks_equal(mask, o[:3]) == [0, 0, 0], (name, c, m, "stand-alone", _masks_equal(mask, o[:3]))
        for q in (False, True):
            fused = vq_forward_route(z, w, 0.25, True, e16, e8, c, m, per_image=True, pixels=xd, refine_queues=q)[3]
            assert _masks_equal(fused, o[:3]) == [0, 0, 0], (name, c, m, "fused", q, _masks_equal(fused, o[:3]))


def test_router_big_from_pixels_with_nan_pixels():
    """a batch-global segment that leaves the workgroup: 16 images of 256x256 are refined as a chain of launches over patched copies
    of the maps (router_big)"""
    B = 16
    assert cg._lib.lib().cgic_router_refine_supported(B, 16, 16, 0) == 1 and cg._lib.lib().cgic_router_refine_in_lds(B, 16, 16, 0) == 0
    x, a8, a16 = _pixel_case("flat_edges", B, 256, 256)
    xd = _t(x)
    e8, e16 = cg.entropy_maps(xd)
    assert np.array_equal(np.isnan(e8.cpu().numpy()), np.isnan(a8)) and np.array_equal(np.isnan(e16.cpu().numpy()), np.isnan(a16))
    for c, m in ((0.1, 0.8), (0.0, 0.4), (0.3, 0.7)):
        o = orc.router(a16, a8, c, m, per_image=False, want_gate=False)
        mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=False)(e16, e8, want_gate=False, pixels=xd)
        assert mode == o[4] and _masks_equal(mask, o[:3]) == [0, 0, 0], (c, m, _masks_equal(mask, o[:3]))


# ---------------------------------------------------------------------------- rate_table
@pytest.mark.parametrize("per_image", [True, False])
@pytest.mark.parametrize("si", range(NS))
def test_rate_table_on_special_maps(golden, si, per_image):
    _, codec, lens = _zipf()
    B, h16, w16 = sr.SHAPES[si]
    inds, hinds = _heads_indices(B, h16, w16, 100 + si)
    for cls in sr.CLASSES:
        e16, e8 = _fixture(golden, si, cls)
        tab = cg.rate_table(codec, *inds, _t(e16), _t(e8), sr.RATIOS, per_image=per_image)
        nb = tab.nbytes.cpu().numpy()
        for ci, (c, m) in enumerate(sr.RATIOS):
            omc, omm, omf, _, mode = orc.router(e16, e8, c, m, per_image=per_image, want_gate=False)
            assert tab.modes[ci] == mode
            for b in range(B):
                want = sr.stream_sizes(omc[b, 0] == 1, omm[b, 0] == 1, omf[b, 0] == 1, hinds[0][b], hinds[1][b], hinds[2][b], lens,
                                       orc.mode_streams(mode))
                assert nb[ci, b].tolist() == want, (si, cls, c, m, b, nb[ci, b].tolist(), want)


# ---------------------------------------------------------------------------- rate_curve
def _curve_raw(table, inds, d16, d8, coarse):
    """cgic_rate_curve -> (nbytes [B, n8 + 1, 5], the workspace summary [B, 4]) as numpy"""
    B, h16, w16 = d16.shape
    n8 = 4 * h16 * w16
    ws = torch.zeros(max(int(_lib.lib().cgic_rate_curve_workspace_bytes(B, h16, w16)), 16), dtype=torch.uint8, device=DEV)
    nb = torch.empty((B, n8 + 1, 5), dtype=torch.int32, device=DEV)
    _lib.call("cgic_rate_curve", rate._table_handle(table), _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]), _lib.ptr(d16),
              _lib.ptr(d8), B, h16, w16, float(coarse), _lib.ptr(nb), _lib.ptr(ws), _lib.current_stream())
    return nb.cpu().numpy(), ws[:B * 16].view(torch.int32).view(B, 4).cpu().numpy()


def _assert_curve(table, lens, inds, hinds, e16, e8, Ks_of, what):
    """the curve of every coarse ratio == curve_at_ranks at the ranks Ks_of(image's sorted medium list) picks"""
    d16, d8 = _t(e16), _t(e8)
    B, h16, w16 = e16.shape
    n16 = h16 * w16
    for c in sr.CURVE_COARSE:
        nb, summary = _curve_raw(table, inds, d16, d8, c)
        k_c, streams = sr.coarse_rank(n16, c), orc.mode_streams(0 if c > 0 else 1)
        for b in range(B):
            Ks = Ks_of(e16[b], e8[b], k_c)
            rows, want_summary = sr.curve_at_ranks(e16[b], e8[b], hinds[0][b], hinds[1][b], hinds[2][b], lens, k_c, Ks, streams)
            got = nb[b, Ks].tolist()
            wrong = [(K, g, r) for K, g, r in zip(Ks, got, rows) if g != r]
            assert not wrong, (what, c, b, len(wrong), wrong[:3])
            assert (summary[b].astype(np.int64) & 0xFFFFFFFF).tolist() == want_summary, (what, c, b, summary[b], want_summary)


def _every_rank(e16, e8, k_c):
    return list(range(e8.size + 1))


def _edge_ranks(e16, e8, k_c):
    """the ends, every rank next to a boundary between two values of the sorted medium list, and every 97th rank"""
    v = np.sort(sr.route_at_ranks(e16, e8, k_c, 0)[3]["v"], axis=None)
    n8 = v.size
    step = np.flatnonzero(v[1:].view(np.uint32) != v[:-1].view(np.uint32)) + 1      # index of the first element of each run
    Ks = {0, 1, 2, n8 - 1, n8} | set(range(0, n8 + 1, 97))
    for i in step.tolist():
        Ks |= {i - 1, i, i + 1, i + 2}
    return sorted(K for K in Ks if 0 <= K <= n8)


@pytest.mark.parametrize("si", range(NS))
def test_rate_curve_on_the_fixture_maps(golden, si):
    _, codec, lens = _zipf()
    B, h16, w16 = sr.SHAPES[si]
    inds, hinds = _heads_indices(B, h16, w16, 200 + si)
    for cls in sr.CLASSES:
        e16, e8 = _fixture(golden, si, cls)
        _assert_curve(codec, lens, inds, hinds, e16, e8, _every_rank, (si, cls))
        # the Python front end on the same maps: n_coarse, and the curve == the rate table at the ranks a ratio reaches
        d16, d8 = _t(e16), _t(e8)
        for c in (0.3, 0.0):
            curve = cg.rate_curve(codec, *inds, d16, d8, c)
            k_c = sr.coarse_rank(h16 * w16, c)
            assert curve.n_coarse.tolist() == [int(sr.route_at_ranks(e16[b], e8[b], k_c, 0)[0].sum()) for b in range(B)]
            pick = curve.ranks[::max(1, len(curve.ranks) // 8)]
            tab = cg.rate_table(codec, *inds, d16, d8, [curve.ratio(K) for K in pick], per_image=True)
            assert torch.equal(curve.nbytes[:, torch.tensor(pick, device=DEV)], tab.nbytes.permute(1, 0, 2)), (si, cls, c)


@pytest.mark.parametrize("cls", sr.CLASSES)
@pytest.mark.parametrize("h16,w16", [(16, 16), (16, 17)])
def test_rate_curve_at_one_element_per_thread_and_just_past(cls, h16, w16):
    """n8 = 1024 (one element per thread of the sort) and 1088: every rank"""
    _, codec, lens = _zipf()
    inds, hinds = _heads_indices(1, h16, w16, 300 + w16)
    e16, e8 = sr.special_maps(1, h16, w16, cls, seed=w16, levels=12)
    _assert_curve(codec, lens, inds, hinds, e16, e8, _every_rank, (cls, h16, w16))


@pytest.mark.parametrize("table", ["zipf", "big"])
@pytest.mark.parametrize("cls", sr.CLASSES)
def test_rate_curve_at_the_limit(cls, table):
    """48x64 coarse patches: n8 = 12 288, the most one workgroup's LDS holds.  With the 1024-symbol table the code lengths are staged
    in LDS behind the words, with 4096 symbols they are read from global memory"""
    h16, w16 = 48, 64
    n8 = 4 * h16 * w16
    if table == "zipf":
        codec, lens, nsym = _zipf()[1], _zipf()[2], 1024
    else:
        coder, lens = _big_table()
        codec, nsym = coder.table.handle, 4096                       # (the rate calls take a GrainCodec or the table's handle)
    assert sr.curve_staged(n8, nsym) == (table == "zipf") and sr.curve_staged(n8, 2048) and not sr.curve_staged(n8, 2049)
    inds, hinds = _heads_indices(1, h16, w16, 400, nsym)
    e16, e8 = sr.special_maps(1, h16, w16, cls, seed=64, levels=40)
    _assert_curve(codec, lens, inds, hinds, e16, e8, _edge_ranks, (cls, table))
    if table == "zipf":
        d16, d8 = _t(e16), _t(e8)
        curve = cg.rate_curve(codec, *inds, d16, d8, 0.3)
        pick = curve.ranks[::max(1, len(curve.ranks) // 16)]
        tab = cg.rate_table(codec, *inds, d16, d8, [curve.ratio(K) for K in pick], per_image=True)
        assert torch.equal(curve.nbytes[:, torch.tensor(pick, device=DEV)], tab.nbytes.permute(1, 0, 2)), cls


# ---------------------------------------------------------------------------- the thread steps of the curve launch
STEP_SHAPES = [(8, 16), (3, 43)]            # n8 = 512: the largest image sorted by 256 threads; 516: the smallest sorted by 512


@functools.lru_cache(maxsize=None)
def _step_case(h16, w16):
    inds, hinds = _heads_indices(2, h16, w16, 700 + w16)
    e16, e8 = sr.special_maps(2, h16, w16, "mix", seed=w16, levels=12)
    return inds, hinds, e16, e8


@pytest.mark.parametrize("h16,w16", STEP_SHAPES)
def test_rate_entry_points_at_the_thread_steps(h16, w16):
    """B = 2 on either side of the step from 256 to 512 threads (16x16, 16x17 and 48x64 are above): the curve at every rank, the
    budget route and a two-shape tiled call, all integers, all exact"""
    _, codec, lens = _zipf()
    inds, hinds, e16, e8 = _step_case(h16, w16)
    d16, d8 = _t(e16), _t(e8)
    B, n16 = 2, h16 * w16
    # ---- the curve: every rank against the reference at explicit ranks, and the CPU oracle's router and sizes at every rank a
    # ratio reaches
    _assert_curve(codec, lens, inds, hinds, e16, e8, _every_rank, (h16, w16))
    for coarse in (0.3, 0.0):
        curve = cg.rate_curve(codec, *inds, d16, d8, coarse)
        nb = curve.nbytes.cpu().numpy()
        assert curve.ranks == list(range(round(4 * n16 * coarse), 4 * n16 + 1))
        for K, (c, m) in zip(curve.ranks, curve.candidates):
            omc, omm, omf, _, mode = orc.router(e16, e8, c, m, per_image=True, want_gate=False)
            for b in range(B):
                want = sr.stream_sizes(omc[b, 0] == 1, omm[b, 0] == 1, omf[b, 0] == 1, hinds[0][b], hinds[1][b], hinds[2][b], lens,
                                       orc.mode_streams(mode))
                assert nb[b, K].tolist() == want, (coarse, K, b, nb[b, K].tolist(), want)
    # ---- the budget route: the router's masks and the merged indices at the rank it reports
    for coarse in (0.3, 0.0):
        Kt, mediums = rate.reachable_ranks_vec(n16, float(coarse))
        ranks = Kt.tolist()
        k_c, streams = sr.coarse_rank(n16, coarse), orc.mode_streams(0 if coarse > 0 else 1)
        per = [sr.curve_at_ranks(e16[b], e8[b], hinds[0][b], hinds[1][b], hinds[2][b], lens, k_c, ranks, streams)[0] for b in range(B)]
        S = [sum(sum(per[b][j]) for b in range(B)) for j in range(len(ranks))]
        for budget in _budgets(S):
            route = cg.route_to_bpp(codec, *inds, d16, d8, coarse, budget=torch.tensor([budget], dtype=torch.int64, device=DEV))
            j = _assert_route(route, hinds, e16, e8, ranks, k_c, per, S, budget, codec, coarse, (h16, w16, coarse))
            o = orc.router(e16, e8, coarse, float(mediums[j]), per_image=True, want_gate=False)
            assert _masks_equal(route.masks, o[:3]) == [0, 0, 0], (coarse, budget, j)
    # ---- one tile of each of the two shapes in one call, both of one image: every tile its own curve, the image their sum
    for coarse in (0.3, 0.0):
        groups, singles = [], []
        for h, w in ((h16, w16), STEP_SHAPES[1 - STEP_SHAPES.index((h16, w16))]):
            ti, _, t16, t8 = _step_case(h, w)
            one, t16, t8 = tuple(t[:1] for t in ti), _t(t16[:1]), _t(t8[:1])
            groups.append((*one, t16, t8, [0]))
            singles.append(_curve_raw(codec, one, t16, t8, coarse)[0][0])
        curve = cg.rate_curve_tiled(codec, groups, coarse, ends=False)
        tile_nb = curve.tile_nbytes.cpu().numpy()
        assert tile_nb.shape == (2, len(curve.candidates), 5) and curve.tile_shape == [0, 1] and len(curve.candidates) >= 16
        fold = np.zeros(tile_nb.shape[1:], np.int64)
        for s, single in enumerate(singles):
            assert np.array_equal(tile_nb[s], single[curve.ranks[s].tolist()]), (coarse, s)
            fold += tile_nb[s]
        assert int(tile_nb.min()) >= 0 and np.array_equal(curve.nbytes.numpy()[0], fold)


# ---------------------------------------------------------------------------- rate_curve_tiled
TILE_SHAPES = [0, 2, 3]            # of sr.SHAPES: 1x1, 3x5 and 4x4 coarse patches


@pytest.mark.parametrize("coarse", [0.3, 0.0])
@pytest.mark.parametrize("cls", sr.CLASSES)
def test_rate_curve_tiled_on_special_maps(golden, cls, coarse):
    """one call with tiles of three shapes: every tile == the single-shape curve == the reference, the image sums == the fold"""
    _, codec, lens = _zipf()
    groups, per_tile = [], []
    images = {0: [0], 2: [1], 3: [0, 1]}
    for si in TILE_SHAPES:
        B, h16, w16 = sr.SHAPES[si]
        inds, hinds = _heads_indices(B, h16, w16, 500 + si)
        e16, e8 = _fixture(golden, si, cls)
        d16, d8 = _t(e16), _t(e8)
        groups.append((*inds, d16, d8, images[si]))
        single = _curve_raw(codec, inds, d16, d8, coarse)[0]
        for b in range(B):
            per_tile.append((si, b, e16[b], e8[b], [h[b] for h in hinds], single[b], images[si][b]))
    curve = cg.rate_curve_tiled(codec, groups, coarse, image_hw=(96, 128), ends=False)        # (two images of different tile sets)
    tile_nb = curve.tile_nbytes.cpu().numpy()
    M = len(curve.candidates)
    assert M >= 16 and tile_nb.shape == (len(per_tile), M, 5)
    fold = np.zeros((2, M, 5), np.int64)
    streams = orc.mode_streams(0 if coarse > 0 else 1)
    for t, (si, b, e16, e8, hi, single, image) in enumerate(per_tile):
        s = TILE_SHAPES.index(si)
        Ks = curve.ranks[s].tolist()
        n16 = e16.size
        assert curve.tile_shape[t] == s and curve.tile_image[t] == image
        assert np.array_equal(tile_nb[t], single[Ks]), (cls, coarse, t, "the single-shape curve")
        rows, _ = sr.curve_at_ranks(e16, e8, *hi, lens, sr.coarse_rank(n16, coarse), Ks, streams)
        assert tile_nb[t].tolist() == rows, (cls, coarse, t, "the reference")
        fold[image] += tile_nb[t]
    assert np.array_equal(curve.nbytes.numpy(), fold)


# ---------------------------------------------------------------------------- route_to_bpp
def _pick(S, budget):
    """cgic_route_to_budget's rule on the batch sizes S[j]: the largest S <= budget (tie: the smaller j); none fits: the smallest S"""
    fit = [j for j in range(len(S)) if S[j] <= budget]
    if fit:
        return min(fit, key=lambda j: (-S[j], j)), 1
    return min(range(len(S)), key=lambda j: (S[j], j)), 0


def _route_case(golden, si, cls, coarse):
    _, codec, lens = _zipf()
    B, h16, w16 = sr.SHAPES[si]
    n16 = h16 * w16
    inds, hinds = _heads_indices(B, h16, w16, 600 + si)
    e16, e8 = _fixture(golden, si, cls)
    K, _ = rate.reachable_ranks_vec(n16, float(coarse))
    ranks = K.tolist()
    k_c, streams = sr.coarse_rank(n16, coarse), orc.mode_streams(0 if coarse > 0 else 1)
    per = [sr.curve_at_ranks(e16[b], e8[b], hinds[0][b], hinds[1][b], hinds[2][b], lens, k_c, ranks, streams)[0] for b in range(B)]
    S = [sum(sum(per[b][j]) for b in range(B)) for j in range(len(ranks))]
    return codec, inds, hinds, e16, e8, ranks, k_c, per, S


def _assert_route(route, hinds, e16, e8, ranks, k_c, per, S, budget, codec, coarse, what):
    j, fits = _pick(S, budget)
    K = ranks[j]
    assert route.choice.cpu().tolist() == [j, K, fits, S[j]], (what, budget, route.choice.cpu().tolist(), [j, K, fits, S[j]])
    B = e16.shape[0]
    mc, mm, mf = (t.cpu().numpy() for t in route.masks)
    ind = route.ind.cpu().numpy()
    assert np.array_equal(sr.up(mc, 4) + sr.up(mm, 2) + mf, np.ones_like(mf))
    for b in range(B):
        gc, gm, gf, _ = sr.route_at_ranks(e16[b], e8[b], k_c, K)
        assert np.array_equal(mc[b, 0], gc.astype(np.int32)) and np.array_equal(mm[b, 0], gm.astype(np.int32)) \
            and np.array_equal(mf[b, 0], gf.astype(np.int32)), (what, budget, b)
        assert np.array_equal(ind[b], sr.merged_indices(hinds[0][b], hinds[1][b], hinds[2][b], gm, gf)), (what, budget, b)
    assert route.mode == (0 if coarse > 0 else 1)
    # compress writes exactly the promised bytes, and both decoders return ind
    comp = codec.compress(route.ind, route.masks, route.mode)
    assert comp.nbytes.clamp(min=0).cpu().tolist() == [per[b][j] for b in range(B)], (what, budget)
    for decoder in ("latency", "throughput"):
        with cg.decoder_mode(decoder):
            dind, _, _, status = codec.decompress(comp)
        assert int(status.abs().max()) == 0 and torch.equal(dind.reshape(route.ind.shape), route.ind), (what, budget, decoder)
    return j


def _budgets(S):
    """budgets that select the first, the last and two interior requested ranks where the rule allows it, and one nothing fits"""
    R = len(S)
    return [S[j] for j in sorted({0, R // 3, (2 * R) // 3, R - 1})] + [min(S) - 1]


@pytest.mark.parametrize("coarse", [0.3, 0.0])
@pytest.mark.parametrize("si", range(NS))
def test_route_to_bpp_on_special_maps(golden, si, coarse):
    for cls in sr.CLASSES:
        codec, inds, hinds, e16, e8, ranks, k_c, per, S = _route_case(golden, si, cls, coarse)
        d16, d8 = _t(e16), _t(e8)
        seen = set()
        for budget in _budgets(S):
            route = cg.route_to_bpp(codec, *inds, d16, d8, coarse, budget=torch.tensor([budget], dtype=torch.int64, device=DEV))
            seen.add((_assert_route(route, hinds, e16, e8, ranks, k_c, per, S, budget, codec, coarse, (si, cls, coarse)), route.fits))
        assert any(not f for _, f in seen) and any(f for _, f in seen)


def test_route_to_bpp_on_special_maps_in_a_captured_graph(golden):
    si, cls, coarse = 4, "mix", 0.3
    codec, inds, hinds, e16, e8, ranks, k_c, per, S = _route_case(golden, si, cls, coarse)
    d16, d8 = _t(e16), _t(e8)
    budget = torch.zeros(1, dtype=torch.int64, device=DEV)
    cg.route_to_bpp(codec, *inds, d16, d8, coarse, budget=budget)        # (the rank list and the code table are uploaded once)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        route = cg.route_to_bpp(codec, *inds, d16, d8, coarse, budget=budget)
    for bud in _budgets(S)[1:]:
        budget.copy_(torch.tensor([bud], dtype=torch.int64))
        g.replay()
        route.refresh()
        _assert_route(route, hinds, e16, e8, ranks, k_c, per, S, bud, codec, coarse, "replay")
