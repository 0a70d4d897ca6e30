"""CPU: the plain reference at explicit ranks (tests/specials_ref.py) on entropy maps that hold NaN, +-Inf, negatives, signed zeros
and denormals -- pinned against the oracle's router (itself pinned to the real router by tests/golden/router_specials.npz) at
every rank a ratio reaches and against the oracle's coder, and a check that every map class exercises what it is there for."""
import numpy as np
import pytest

import control_gic_amd as cg
from control_gic_amd import rate
import specials_ref as sr
from oracle import cgic_oracle as orc


def _cases(golden):
    g = golden("router_specials")
    for si, shape in enumerate(sr.SHAPES):
        for cls in sr.CLASSES:
            yield si, shape, cls, g[f"s{si}_{cls}_e16"], g[f"s{si}_{cls}_e8"]


def test_fixture_maps_are_the_generators(golden):
    """the committed maps are special_maps' (bit for bit, NaN payloads included): the GPU tests may plant the same classes elsewhere"""
    for si, (B, h16, w16), cls, e16, e8 in _cases(golden):
        w16_, w8_ = sr.special_maps(B, h16, w16, cls, seed=1000 * si + sr.CLASSES.index(cls))
        assert np.array_equal(e16.view(np.uint32), w16_.view(np.uint32)) and np.array_equal(e8.view(np.uint32), w8_.view(np.uint32))


def test_route_at_ranks_is_the_oracle_router_at_every_reachable_rank(golden):
    checked = 0
    for si, (B, h16, w16), cls, e16, e8 in _cases(golden):
        n16 = h16 * w16
        for c in (0.0, 0.1, 0.3, 0.5):
            for K, m in rate.reachable_ranks(n16, c):
                k_c, k_m = cg.router_ranks(c, m, n16)
                assert k_m == K and k_c == sr.coarse_rank(n16, c)
                omc, omm, omf, _, mode = orc.router(e16, e8, c, m, per_image=True)
                assert mode == (0 if c > 0 else 1)
                for b in range(B):
                    gc, gm, gf, _ = sr.route_at_ranks(e16[b], e8[b], k_c, K)
                    assert np.array_equal(gc, omc[b, 0] == 1) and np.array_equal(gm, omm[b, 0] == 1) and np.array_equal(gf, omf[b, 0] == 1), \
                        (si, cls, c, K, b)
                    checked += 1
        # the flattened batch is one segment of B * n16 patches
        for c, m in ((0.1, 0.8), (0.3, 0.3), (0.0, 0.4)):
            k_c, K = cg.router_ranks(c, m, B * n16)
            omc, omm, omf, _, _ = orc.router(e16, e8, c, m, per_image=False)
            gc, gm, gf, _ = sr.route_at_ranks(e16, e8, k_c, K)
            assert np.array_equal(gc, omc[:, 0] == 1) and np.array_equal(gm, omm[:, 0] == 1) and np.array_equal(gf, omf[:, 0] == 1)
    assert checked > 2000


def test_sizes_are_the_oracle_coders(golden):
    """stream_sizes / merged_indices == len(orc.compress_image(...)) of the oracle's select and coder, at sampled reachable ranks"""
    htab = orc.HuffmanTable(sr.FREQ)
    rng = np.random.default_rng(5)
    for si, (B, h16, w16), cls, e16, e8 in _cases(golden):
        n16 = h16 * w16
        inds = [rng.integers(0, 1024, (B, s * h16, s * w16)).astype(np.int64) for s in (1, 2, 4)]
        for c in (0.0, 0.3):
            ranks = rate.reachable_ranks(n16, c)
            mode = 0 if c > 0 else 1
            for K, m in ranks[::max(1, len(ranks) // 6)]:
                k_c = sr.coarse_rank(n16, c)
                for b in range(B):
                    gc, gm, gf, _ = sr.route_at_ranks(e16[b], e8[b], k_c, K)
                    ic, im, if_ = (t[b] for t in inds)
                    ind = sr.merged_indices(ic, im, if_, gm, gf)
                    streams = orc.compress_image(ind, gc.astype(np.int32), gm.astype(np.int32), gf.astype(np.int32), mode, htab)
                    want = [len(streams[n]) if n in streams else 0 for n in orc.STREAM_NAMES]
                    assert sr.stream_sizes(gc, gm, gf, ic, im, if_, htab.len, orc.mode_streams(mode)) == want, (si, cls, c, K, b)
                    rows, summary = sr.curve_at_ranks(e16[b], e8[b], ic, im, if_, htab.len, k_c, [K], orc.mode_streams(mode))
                    assert rows == [want] and summary[0] == int(gc.sum())


def test_curve_at_ranks_is_route_at_ranks_at_every_rank(golden):
    """the curve's reference (the part that does not depend on K done once) == stream_sizes of route_at_ranks, at EVERY rank -- also
    the ranks no ratio reaches -- and every coarse ratio of the curve tests, 1.0 included"""
    htab = orc.HuffmanTable(sr.FREQ)
    rng = np.random.default_rng(6)
    for si, (B, h16, w16), cls, e16, e8 in _cases(golden):
        n16 = h16 * w16
        ic, im, if_ = (rng.integers(0, 1024, (s * h16, s * w16)).astype(np.int64) for s in (1, 2, 4))
        for c in sr.CURVE_COARSE:
            k_c, streams = sr.coarse_rank(n16, c), orc.mode_streams(0 if c > 0 else 1)
            Ks = list(range(4 * n16 + 1))
            rows, summary = sr.curve_at_ranks(e16[0], e8[0], ic, im, if_, htab.len, k_c, Ks, streams)
            for K in Ks:
                gc, gm, gf, info = sr.route_at_ranks(e16[0], e8[0], k_c, K)
                assert rows[K] == sr.stream_sizes(gc, gm, gf, ic, im, if_, htab.len, streams), (si, cls, c, K)
            assert summary[:2] == [int(gc.sum()), sr.threshold_bits(info["tc"], k_c)]


@pytest.mark.parametrize("cls", sr.CLASSES)
def test_every_class_exercises_what_it_is_there_for(golden, cls):
    """over the fixture's shapes, the curve's coarse ratios and EVERY medium rank: each property the class is required to reach
    (specials_ref.REQUIRED: a NaN threshold, a negative one, a NaN product in the medium list, ...) holds at some (k_c, K)"""
    g = golden("router_specials")
    seen = set()
    for si, (B, h16, w16) in enumerate(sr.SHAPES):
        e16, e8 = g[f"s{si}_{cls}_e16"], g[f"s{si}_{cls}_e8"]
        n16 = h16 * w16
        for b in range(B):
            for k_c in sorted({sr.coarse_rank(n16, c) for c in sr.CURVE_COARSE}):
                for K in range(4 * n16 + 1):
                    seen |= sr.properties(e16[b], e8[b], k_c, K)
    assert sr.REQUIRED[cls] <= seen, (cls, sorted(sr.REQUIRED[cls] - seen))


def test_threshold_bits():
    assert sr.threshold_bits(np.float32(-0.0), 3) == 0 and sr.threshold_bits(np.float32("nan"), 1) == 0x7FC00000
    assert sr.threshold_bits(np.float32(1.0), 0) == 0 and sr.threshold_bits(np.float32(1.0), 2) == 0x3F800000
    assert sr.threshold_bits(np.float32(-np.inf), 2) == 0xFF800000 and sr.threshold_bits(sr.DEN, 1) == int(sr.DEN.view(np.uint32))
