"""Entropy maps holding NaN, +-Inf, negatives, signed zeros and denormals, and a plain numpy reference of the router at EXPLICIT
ranks on them -- test infrastructure shared by tests/golden/make_golden_specials.py, tests/test_specials_host.py and
tests/test_special_entropies.py.

The router (RouterTriple.py:21-34) decides on k-th smallest entropies with a strict float '<'.  The rate curve answers every medium
rank K, not only the ranks a ratio reaches, so the checker takes the ranks themselves: `route_at_ranks` is np.sort (NaN last, like
torch.sort), s[k - 1 if k else 0], the fp32 product e8 * (1 - gate) and float '<', nothing else.  Masks, merged indices and the five
stream sizes (the byte formula of tests/test_rate_control_host.py on a table's code lengths) follow from it.
"""
import numpy as np

SHAPES = [(1, 1, 1), (1, 1, 3), (1, 3, 5), (2, 4, 4), (3, 2, 7)]
CLASSES = ["nan_e8", "nan_pixels", "gated", "inf", "neg", "zeros", "all_nan", "all_equal", "mix"]
RATIOS = [(0.1, 0.8), (0.3, 0.3), (0.5, 0.45), (0.0, 0.4), (0.4, 0.0), (0.3, 0.7), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)]
CURVE_COARSE = [0.0, 0.1, 0.3, 0.5, 1.0]
NAN, INF = np.float32(np.nan), np.float32(np.inf)
DEN = np.float32(1e-40)
MIX = np.array([NAN, INF, -INF, 0.0, -0.0, -1.5, DEN, -DEN], np.float32)
FREQ = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)


def up(a, k):
    return np.repeat(np.repeat(a, k, -2), k, -1)


def _some(rng, n, frac):
    """a random subset of range(n): about frac of it, at least one element"""
    return rng.permutation(n)[:max(1, int(round(n * frac)))]


def plant(e16, e8, cls, rng):
    """plant the special values of class `cls` into the maps [B,h16,w16] / [B,2h16,2w16], in place.  Every special value is planted
    more than once where the map has room (exact ties), and the seeded values around them come from a handful of levels"""
    B, h16, w16 = e16.shape
    f16, f8 = e16.reshape(-1), e8.reshape(-1)
    if cls == "nan_e8":
        f8[_some(rng, f8.size, 1 / 6)] = NAN
    elif cls == "nan_pixels":
        # as entropy_maps makes them: a NaN pixel is a NaN 16x16 patch and a NaN in one or more of its 8x8 patches
        for p in _some(rng, f16.size, 1 / 6):
            b, r = divmod(int(p), h16 * w16)
            y, x = divmod(r, w16)
            e16[b, y, x] = NAN
            kids = _some(rng, 4, rng.integers(1, 5) / 4)
            for q in kids:
                e8[b, 2 * y + q // 2, 2 * x + q % 2] = NAN
    elif cls == "gated":
        # NaN / +Inf in e8 under the two patches of each image that turn coarse first (the two smallest e16, both distinct)
        kids = np.array([[NAN, INF, 0.5, NAN], [INF, 0.25, INF, -0.5]], np.float32)
        for b in range(B):
            order = rng.permutation(h16 * w16)[:2]
            for j, r in enumerate(order):
                y, x = divmod(int(r), w16)
                e16[b, y, x] = (0.0625, 0.125)[j]
                e8[b, 2 * y:2 * y + 2, 2 * x:2 * x + 2] = kids[j].reshape(2, 2)
    elif cls == "inf":
        for f in (f16, f8):
            idx = _some(rng, f.size, 1 / 3)
            f[idx] = np.where(np.arange(idx.size) % 2 == 0, INF, -INF)
    elif cls == "neg":
        vals = np.array([-1.5, -INF, -0.25, -1.5], np.float32)
        for f in (f16, f8):
            idx = _some(rng, f.size, 1 / 2)
            f[idx] = vals[np.arange(idx.size) % 4]
    elif cls == "zeros":
        vals = np.array([0.0, -0.0, DEN, -DEN], np.float32)
        for f in (f16, f8):
            idx = _some(rng, f.size, 2 / 3)
            f[idx] = vals[np.arange(idx.size) % 4]
    elif cls == "all_nan":
        f16[:] = NAN
        f8[:] = NAN
    elif cls == "all_equal":
        f16[:] = 0.75
        f8[:] = 0.75
    elif cls == "mix":
        for f in (f16, f8):
            idx = _some(rng, f.size, 1 / 2)
            f[idx] = MIX[rng.integers(0, MIX.size, idx.size)]
    else:
        raise ValueError(cls)


def special_maps(B, h16, w16, cls, seed, levels=6):
    """(e16 [B,h16,w16], e8 [B,2h16,2w16]) float32: seeded values on `levels` levels (planted ties) with class `cls` planted"""
    rng = np.random.default_rng(seed)
    e16 = (rng.integers(1, levels + 1, (B, h16, w16)) / 4).astype(np.float32)
    e8 = (rng.integers(1, levels + 3, (B, 2 * h16, 2 * w16)) / 4).astype(np.float32)
    plant(e16, e8, cls, rng)
    return e16, e8


def fixture_masks(g, si, cls):
    """the masks of tests/golden/router_specials.npz for shape si and class cls -> {(ri, "batch" | "per"): (mc, mm, mf) int32 in the
    router's layouts [B,1,.,.]}, in the order make_golden_specials.py packed them"""
    B, h16, w16 = SHAPES[si]
    shapes = [(B, 1, h16, w16), (B, 1, 2 * h16, 2 * w16), (B, 1, 4 * h16, 4 * w16)]
    bits = np.unpackbits(g[f"s{si}_{cls}_masks"])
    out, at = {}, 0
    for ri in range(len(RATIOS)):
        for how in ("batch", "per"):
            ms = []
            for shp in shapes:
                n = int(np.prod(shp))
                ms.append(bits[at:at + n].astype(np.int32).reshape(shp))
                at += n
            out[(ri, how)] = tuple(ms)
    assert at <= bits.size < at + 8
    return out


def route_at_ranks(e16, e8, k_c, K):
    """RouterTriple.py:21-34 on ONE segment (all of e16 [.., h16, w16] / e8 [.., 2h16, 2w16] flattened) at explicit ranks: coarse rank
    k_c (0: the threshold is s16[0], nothing is below it -- also what mode 1 does) and medium rank K
    -> (mask_c, mask_m, mask_f bool, info: the thresholds tc / tm, the medium list v, the coarse gate on the 8x8 grid)"""
    e16, e8 = np.asarray(e16, np.float32), np.asarray(e8, np.float32)
    s16 = np.sort(e16, axis=None)                                      # NaN last
    tc = s16[k_c - 1 if k_c else 0]
    gc = e16 < tc
    g8 = up(gc, 2)
    with np.errstate(invalid="ignore"):
        v = e8 * (np.float32(1) - g8.astype(np.float32))             # the fp32 product: NaN * 0 and Inf * 0 are NaN
    assert v.dtype == np.float32
    sv = np.sort(v, axis=None)
    tm = sv[K - 1 if K else 0]
    gm = (e8 < tm) & ~g8
    gf = ~up(gc, 4) & ~up(gm, 2)
    return gc, gm, gf, dict(tc=tc, tm=tm, v=v, g8=g8)


def merged_indices(ind_c, ind_m, ind_f, gm, gf):
    """cgic_gather_grain_indices: mask_f ? ind_f : up2(mask_m) ? up2(ind_m) : up4(ind_c)"""
    return np.where(gf, ind_f, np.where(up(gm, 2), up(ind_m, 2), up(ind_c, 4)))


def file_bytes(count, bits):
    """HuffmanCoding.compress: no symbols -> an empty file; else a header byte + the bits padded by 1..8 zero bits"""
    return 0 if count == 0 else int(bits) // 8 + 2


def stream_sizes(gc, gm, gf, ind_c, ind_m, ind_f, lens, streams):
    """the five .bin sizes of ONE image from its masks; streams: five bools (which files the mode writes; others 0)"""
    out = [file_bytes(int(gc.sum()), lens[ind_c[gc]].sum()), file_bytes(int(gm.sum()), lens[ind_m[gm]].sum()),
           file_bytes(int(gf.sum()), lens[ind_f[gf]].sum()), gc.size // 8 + 2, gm.size // 8 + 2]
    return [s if on else 0 for s, on in zip(out, streams)]


def threshold_bits(t, k):
    """what the curve's workspace summary holds for the coarse threshold: its fp32 bit pattern with +-0 as +0 and any NaN as the
    quiet NaN; 0 without a coarse rank"""
    if not k:
        return 0
    if np.isnan(t):
        return 0x7FC00000
    if t == 0:
        return 0
    return int(np.float32(t).view(np.uint32))


def curve_at_ranks(e16, e8, ind_c, ind_m, ind_f, lens, k_c, Ks, streams):
    """ONE image at coarse rank k_c and every medium rank of Ks -> (nbytes [len(Ks)][5], summary [4] as the curve's workspace holds
    it: coarse patches, threshold_bits of the coarse threshold, medium / fine code bits of all non-coarse patches).  route_at_ranks
    with the part that does not depend on K -- the coarse gate, the medium list and its sort -- done once (the host test holds the
    two to each other at every rank)"""
    e8 = np.asarray(e8, np.float32)
    gc, _, _, info = route_at_ranks(e16, e8, k_c, 0)
    g8, g4 = info["g8"], up(gc, 4)
    sv = np.sort(info["v"], axis=None)
    lm, lf = lens[ind_m], lens[ind_f]
    size_c = file_bytes(int(gc.sum()), lens[ind_c[gc]].sum())
    rows = []
    for K in Ks:
        gm = (e8 < sv[K - 1 if K else 0]) & ~g8
        gf = ~g4 & ~up(gm, 2)
        out = [size_c, file_bytes(int(gm.sum()), lm[gm].sum()), file_bytes(int(gf.sum()), lf[gf].sum()), gc.size // 8 + 2, gm.size // 8 + 2]
        rows.append([s if on else 0 for s, on in zip(out, streams)])
    summary = [int(gc.sum()), threshold_bits(info["tc"], k_c), int(lm[~g8].sum()), int(lf[~g4].sum())]
    return rows, summary


def coarse_rank(n16, c):
    """the curve's coarse rank: Python's round (half-even) of the float64 product; 0 at coarse ratio 0"""
    return round(n16 * c) if c > 0 else 0


def curve_staged(n8, nsym):
    """the curve's launch plan (cgic_rate_plan.h, curve_plan): the code lengths are staged in LDS behind the 12 bytes per 8x8 patch
    when both fit 152 KB (tests/test_rate_plan_host.py holds this to the plan itself)"""
    return 12 * n8 + 4 * nsym <= 152 * 1024


def properties(e16, e8, k_c, K):
    """what a (k_c, K) pair exercises on one segment: the set of names that hold"""
    gc, gm, gf, info = route_at_ranks(e16, e8, k_c, K)
    tc, tm, v, g8 = info["tc"], info["tm"], info["v"], info["g8"]
    e8 = np.asarray(e8, np.float32)
    out = set()
    if k_c and np.isnan(tc): out.add("tc_nan")
    if k_c and tc < 0: out.add("tc_neg")
    if k_c and np.isinf(tc): out.add("tc_inf")
    if k_c and tc == 0: out.add("tc_zero")
    if np.isnan(tm): out.add("tm_nan")
    if tm < 0: out.add("tm_neg")
    if tm == -INF: out.add("tm_neginf")
    if tm == INF: out.add("tm_posinf")
    if tm == 0: out.add("tm_zero")
    if tm != 0 and abs(tm) < np.float32(1.2e-38): out.add("tm_denormal")
    if g8.any():
        out.add("coarse")
        if np.isnan(v[g8]).any(): out.add("nan_product")
        if (np.isinf(e8[g8])).any(): out.add("inf_gated")
        if (e8[g8] < 0).any(): out.add("neg_gated")
        if tm <= 0: out.add("gated_zeros_not_below")
        if tm > 0: out.add("gated_zeros_below")
    if gm.any(): out.add("medium")
    if gf.any(): out.add("fine")
    if np.isnan(e8[~g8]).any() and not np.isnan(tm): out.add("nan_above_threshold")
    if (e8[~g8] == tm).sum() > 1: out.add("tie_at_threshold")
    return out


# what every class must exercise at one (k_c, K) at least, over the fixture's shapes (tests/test_specials_host.py asserts it)
REQUIRED = {
    "nan_e8": {"tm_nan", "nan_above_threshold", "tie_at_threshold"},
    "nan_pixels": {"tc_nan", "tm_nan", "nan_above_threshold", "tie_at_threshold"},
    "gated": {"nan_product", "inf_gated", "neg_gated", "tm_nan", "gated_zeros_below", "tie_at_threshold"},
    "inf": {"tc_inf", "tm_neginf", "tm_posinf", "inf_gated", "nan_product", "tie_at_threshold"},
    "neg": {"tc_neg", "tm_neg", "tm_neginf", "neg_gated", "gated_zeros_not_below", "gated_zeros_below", "tie_at_threshold"},
    "zeros": {"tc_zero", "tm_zero", "tm_denormal", "gated_zeros_not_below", "tie_at_threshold"},
    "all_nan": {"tc_nan", "tm_nan"},
    "all_equal": {"tie_at_threshold", "fine"},
    "mix": {"tc_nan", "tm_nan", "tm_neg", "nan_product", "gated_zeros_not_below", "gated_zeros_below", "tie_at_threshold"},
}
