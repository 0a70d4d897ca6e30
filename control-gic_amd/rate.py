"""Rate control: exact per-ratio rate tables and compress-to-target-bpp.

The bitrate of Control-GIC is set through the granularity ratio (coarse, medium) of the router; which ratio gives which bpp
depends on the image.  `rate_table` answers that for C candidate ratios at once, exactly (the bytes CGIC.compress would write,
model.py:217-262) and without writing a stream: the VQ of each encoder head at its own resolution gives the indices of every
ratio (grain_indices), and a stream's size depends on the masks only through the summed code lengths of the symbols they
select (include/cgic_hip.h, section I).  `compress_to_bpp` then compresses the ratio `choose` picks.

`rate_curve` answers it for EVERY setting of the medium ratio at one coarse ratio: the medium decision of the router is one
integer, the rank K of its threshold among the 8x8-patch entropies, and one sort of the image's patches gives the sizes of all
n8 + 1 ranks (cgic_rate_curve).  `compress_to_bpp(..., search="curve")` picks among all of them.

`route_to_bpp` keeps the decision of that search on the device: the curve at the ranks a ratio reaches, the pick under a byte
budget read from device memory, and the masks and merged indices of the picked rank, in one launch chain without a host
synchronisation (cgic_route_to_budget) -- so a rate-controlled batch can sit inside a captured graph.
`compress_to_bpp(..., search="device")` compresses what it routes.

`rate_curve_tiled` answers it for tiled high-resolution images (highres.py): ONE ratio pair for all tiles of an image, every
tile routed on its own thresholds, so an image's bytes at (c, m) are the sum of its tiles' curves at the rank m gives a tile of
that SHAPE (`tiled_settings`: the medium axis of a set of shapes); one call for all tiles of all shapes
(cgic_rate_curve_tiles).  `compress_tiled_to_bpp` compresses N same-size images at the setting it picks.
"""
import ctypes
import functools
import math

import torch

from . import _lib
from .quantize import FusedQuantConv, _vq_forward
from .router import TripleGrainFixedEntropyRouter, refine_source, routing_per_image

#: the most candidates one rate_table call takes (cgic_rate_table)
MAX_CANDIDATES = 64


def _table_handle(codec):
    """the cgic_table* handle of a code table: from a GrainCodec (codec.huffman.table.handle), or the handle itself -- how the
    torch.ops.cgic rate ops, which carry the table as its handle, reach the same calls"""
    huffman = getattr(codec, "huffman", None)
    return codec if huffman is None else huffman.table.handle


def _head_indices(quantizer, h, quant_conv):
    conv, bias_first = None, False
    fused = isinstance(quant_conv, torch.nn.Conv2d) and tuple(quant_conv.weight.shape) == (4, 4, 1, 1) \
        and quantizer.n_e % 64 == 0 and quantizer.n_e <= 1024
    if quant_conv is not None and not fused:
        h = quant_conv(h)
        if hasattr(h, "materialize"):
            h = h.materialize()
    elif fused:
        conv, bias_first = quant_conv, getattr(quant_conv, "bias_first", FusedQuantConv.bias_first)
    h = h.detach().contiguous().float()
    B, _, hh, ww = h.shape
    idx = _vq_forward(h, quantizer.embedding.weight, quantizer.beta, quantizer.legacy, None, want_zq=False, want_loss=False,
                      quant_conv=conv, conv_bias_first=bias_first, prepared=quantizer._prepared_image())[2]
    return idx.view(B, hh, ww)


def grain_indices(quantizer, h_c, h_m, h_f, quant_conv=None):
    """VQ indices of the three encoder heads (conv_out_coarse / conv_out / conv_out_fine outputs, [B,4,h/4,w/4], [B,4,h/2,w/2],
    [B,4,h,w]) at their own resolutions -> (ind_c, ind_m, ind_f) int64 [B,h/4,w/4], [B,h/2,w/2], [B,h,w].  quant_conv: the model's
    quant_conv (fused into the VQ kernel as install() does), or None.  With finite latents these are the indices the VQ of the
    merged latent gives at the positions each grain owns, for every ratio.  The usage counter / histogram are not touched."""
    if quantizer.training:
        raise RuntimeError("grain_indices: the quantiser is in training mode (its forward would count usage); call .eval() first")
    with torch.no_grad():
        return tuple(_head_indices(quantizer, h, quant_conv) for h in (h_c, h_m, h_f))


def _check_candidates(candidates):
    cand = [(float(c), float(m)) for c, m in candidates]
    if not 1 <= len(cand) <= MAX_CANDIDATES:
        raise ValueError(f"rate_table: {len(cand)} candidates; 1..{MAX_CANDIDATES} are supported")
    return cand


def default_candidates(coarse_ratio, n=16):
    """n candidates with `coarse_ratio` fixed and the medium ratio spread evenly over [0, 1 - coarse], both ends included
    (with coarse > 0: mode 2 at medium = 0, mode 0 inside, mode 3 at the top; coarse = 0 spans modes 6, 1, 5; coarse = 1: mode 4)"""
    n = int(n)
    if not 2 <= n <= MAX_CANDIDATES:
        raise ValueError(f"default_candidates: n={n}; 2..{MAX_CANDIDATES}")
    c = float(coarse_ratio)
    if not 0.0 <= c <= 1.0:
        raise ValueError(f"default_candidates: coarse ratio {c} outside [0, 1]")
    top = 1.0 - c
    return [(c, top * i / (n - 1) if i < n - 1 else top) for i in range(n)]


def _curve_inputs(ind_c, ind_m, ind_f, e16, e8):
    """the input contract of every rate call: everything on one device, the maps as contiguous fp32 [B, h16, w16] and
    [B, 2 h16, 2 w16], the grain indices int64 with the element counts of the three grids
    -> ([ind_c, ind_m, ind_f] contiguous, e16, e8, (B, h16, w16))"""
    _lib.require_device(ind_c, ind_m, ind_f, e16, e8)
    e16c, e8c = e16.contiguous().float(), e8.contiguous().float()
    B, h16, w16 = e16c.shape
    if tuple(e8c.shape) != (B, 2 * h16, 2 * w16):
        raise ValueError(f"e8 {tuple(e8.shape)} must be [B, 2*h16, 2*w16] of {tuple(e16.shape)}")
    want = ((B, h16, w16), (B, 2 * h16, 2 * w16), (B, 4 * h16, 4 * w16))
    inds = []
    for t, shp in zip((ind_c, ind_m, ind_f), want):
        if t.dtype != torch.int64 or t.numel() != shp[0] * shp[1] * shp[2]:
            raise ValueError(f"grain indices must be int64 with shapes {want}")
        inds.append(t.contiguous())
    return inds, e16c, e8c, (B, h16, w16)


class _Rates:
    """what the four results share: bytes (the five streams summed), bpp = bytes * 8 / num_pixels, batch_bpp (all bits of the batch
    over all its pixels), with the images along `image_axis` of bytes; who: the caller's name for the KeyError of a negative entry
    (a symbol outside the code table), None: the entries were checked before"""

    def _set_rates(self, nbytes, num_pixels, image_axis, who):
        self.num_pixels = int(num_pixels)
        self._image_axis = image_axis
        nb = nbytes.detach().cpu()
        if who is not None and nb.numel() and int(nb.min()) < 0:
            raise KeyError(f"{who}: an index is not in the code table")
        self.bytes = nb.to(torch.int64).sum(dim=2)
        self.bpp = self.bytes.to(torch.float64) * 8 / self.num_pixels
        B = self.bytes.shape[image_axis]
        self.batch_bpp = self.bytes.sum(dim=image_axis).to(torch.float64) * 8 / (self.num_pixels * max(B, 1))

    def _choices(self):
        """for choose: (batch_bpp of each candidate, per image the bpp of each candidate, candidate index -> what choose returns)"""
        return self.batch_bpp, (self.bpp.t() if self._image_axis == 1 else self.bpp), int


class RateTable(_Rates):
    """rate_table's result: per candidate and image the sizes of the five .bin streams.
    nbytes int32 [C,B,5] (0 = not written), bytes int64 [C,B], bpp float64 [C,B] (bytes * 8 / pixels, model.py:233),
    batch_bpp float64 [C] (all bits of the batch over all its pixels); candidates: the (coarse, medium) list, modes: their modes"""
    _who = "rate_table"                              # the name in the KeyError of a negative entry (None: not checked)

    def __init__(self, nbytes, candidates, num_pixels):
        self.nbytes = nbytes
        self.candidates = list(candidates)
        self.modes = [int(_lib.lib().cgic_router_mode(c, m)) for c, m in self.candidates]
        self._set_rates(nbytes, num_pixels, 1, self._who)


def rate_table(codec, ind_c, ind_m, ind_f, e16, e8, candidates, per_image=True, pixels=None, flat8=None):
    """exact sizes of the streams GrainCodec.compress would write after routing at each candidate (coarse, medium) ratio
    (cgic_rate_table).  ind_*: grain_indices(...); e16 / e8: the entropy maps; pixels: the image batch behind them (fp32
    [B,3,H,W] or uint8 [B,H,W,3]) for the router's threshold-band refinement -- taken from the maps' tags when they come from
    control_gic_amd.Entropy / entropy_maps, like the router does.  per_image as the router's.  -> RateTable"""
    cand = _check_candidates(candidates)
    inds, e16c, e8c, (B, h16, w16) = _curve_inputs(ind_c, ind_m, ind_f, e16, e8)
    pixels, flat8, explicit = refine_source(e16, e8, pixels, flat8)
    dev = e16c.device
    C = len(cand)
    cr = (ctypes.c_double * C)(*[c for c, _ in cand])
    mr = (ctypes.c_double * C)(*[m for _, m in cand])
    pi = int(bool(per_image))
    px, keep = _lib.pixels_arg(pixels, B, h16, w16, pi, flat8=flat8, queues=False, explicit=explicit)
    nbytes = torch.empty((C, B, _lib.NUM_STREAMS), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(_lib.lib().cgic_rate_table_workspace_bytes(B, h16, w16, C, pi)), 1), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("cgic_rate_table", _table_handle(codec), _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]),
                  _lib.ptr(e16c), _lib.ptr(e8c), B, h16, w16, C, cr, mr, pi, px, _lib.ptr(nbytes), _lib.ptr(ws),
                  _lib.current_stream(dev))
    del keep
    return RateTable(nbytes, cand, 256 * h16 * w16)


def router_ranks(coarse_ratio, medium_ratio, n16):
    """(k_coarse, k_medium) the router derives from a ratio pair for a segment of n16 coarse patches (cgic_router_ranks: Python's
    round on the float64 products; 0 where the mode uses none).  Raises CgicError if k > n, like the router."""
    kc, km = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call("cgic_router_ranks", float(coarse_ratio), float(medium_ratio), int(n16), ctypes.byref(kc), ctypes.byref(km))
    return kc.value, km.value


def ratio_for_rank(K, n16, coarse_ratio):
    """a medium ratio in (0, 1] whose medium rank is K at this coarse ratio, in the curve's mode (0 with coarse > 0, else 1), or
    None if no ratio reaches K there: starts at (K - 4 n16 c) / n8 and steps by one float64 at a time until cgic_router_ranks
    returns K and cgic_router_mode the curve's mode"""
    l = _lib.lib()
    K, n16, c = int(K), int(n16), float(coarse_ratio)
    n8 = 4 * n16
    want = 0 if c > 0.0 else 1
    tiny = math.nextafter(0.0, 1.0)
    m = (K - 4 * n16 * c) / n8
    if m <= 0.0:
        m = tiny
    kc, km = ctypes.c_int64(0), ctypes.c_int64(0)
    for _ in range(64):
        rc = l.cgic_router_ranks(c, m, n16, ctypes.byref(kc), ctypes.byref(km))
        ok = rc == _lib.OK and l.cgic_router_mode(c, m) == want
        if ok and km.value == K:
            return m
        # a rank below K: a larger ratio; above it, k > n, or the fine ratio has reached 0 (modes 3 / 5): a smaller one
        m = math.nextafter(m, 2.0 if (ok and km.value < K) else 0.0)
        if not tiny <= m <= 1.0:
            return None
    return None


@functools.lru_cache(maxsize=64)
def reachable_ranks(n16, coarse_ratio):
    """((K, medium ratio), ...) for every medium rank K in 0 .. n8 a ratio reaches at this coarse ratio: what ratio_for_rank
    returns for each K, from the one search over all of them (reachable_ranks_vec)"""
    K, m = reachable_ranks_vec(n16, coarse_ratio)
    return tuple(zip(K.tolist(), m.tolist()))


def _curve_ranks_vec(coarse_ratio, mediums, n16):
    """cgic_router_ranks + cgic_router_mode for a float64 tensor of medium ratios at once, in the curve's mode -> (ok bool [M],
    k_medium int64 [M]): ok where the pair is in the curve's mode (medium != 0 and 1 - coarse - medium != 0) with 0 <= k <= n8.
    The same float64 operations in the same order as the library's (one product and one sum, round-half-even)"""
    c, n16 = float(coarse_ratio), int(n16)
    n8 = 4 * n16
    m = torch.as_tensor(mediums, dtype=torch.float64)
    fine = (1.0 - c) - m
    k = torch.round(float(4 * n16) * c + float(n8) * m) if c > 0.0 else torch.round(float(n8) * m)
    ok = (m != 0) & (fine != 0) & (k >= 0) & (k <= n8)
    return ok, k.to(torch.int64)


@functools.lru_cache(maxsize=64)
def reachable_ranks_vec(n16, coarse_ratio):
    """every rank searched at once -> (K int64 [R], medium float64 [R]): ratio_for_rank's search (start at (K - 4 n16 c) / n8, step
    one float64 at a time towards the rank) on all n8 + 1 ranks in lockstep, pinned to it bit for bit by a test.  A 768x768 tile
    has 9217 ranks: a loop over ratio_for_rank makes two foreign calls per step, this a handful of tensor operations"""
    n16, c = int(n16), float(coarse_ratio)
    n8 = 4 * n16
    tiny = math.nextafter(0.0, 1.0)
    K = torch.arange(n8 + 1, dtype=torch.int64)
    m = (K.to(torch.float64) - 4 * n16 * c) / n8
    m = torch.where(m <= 0.0, torch.full_like(m, tiny), m)
    found = torch.zeros(n8 + 1, dtype=torch.bool)
    alive = torch.ones(n8 + 1, dtype=torch.bool)
    up, down = torch.full_like(m, 2.0), torch.zeros_like(m)
    for _ in range(64):
        ok, km = _curve_ranks_vec(c, m, n16)
        found |= alive & ok & (km == K)
        alive &= ~found
        if not bool(alive.any()):
            break
        step = torch.nextafter(m, torch.where(ok & (km < K), up, down))
        m = torch.where(alive, step, m)
        alive &= (m >= tiny) & (m <= 1.0)
    return K[found], m[found]


def tiled_settings(shapes_n16, coarse_ratio):
    """the medium axis of a tiled image: shapes_n16 = the number of 16x16 patches of each distinct tile shape ->
    (mediums float64 [M], ranks int64 [S, M]).  mediums: ascending, the union over the shapes of the ratios that reach each of a
    shape's medium ranks (reachable_ranks), all in the curve's mode (0, or 1 at coarse ratio 0) with a positive fine ratio;
    ranks[s, j]: the rank cgic_router_ranks gives a tile of shape s at (coarse_ratio, mediums[j]).  Every shape's row takes every
    rank that shape can reach: no setting of the image is left out"""
    shapes = tuple(int(n) for n in shapes_n16)
    if not shapes or min(shapes) <= 0:
        raise ValueError(f"tiled_settings: shapes_n16={shapes_n16!r}")
    return _tiled_settings(shapes, float(coarse_ratio))


@functools.lru_cache(maxsize=16)
def _tiled_settings(shapes, c):
    per = [reachable_ranks_vec(n, c) for n in shapes]
    m = torch.unique(torch.cat([p[1] for p in per]))                     # sorted, distinct
    # a ratio found a step above 1 - coarse (the start of the top rank's search can round up) has a negative fine ratio: the
    # float64 just below 1 - coarse reaches the same rank
    top = (1.0 - c) - m <= 0
    if bool(top.any()):
        m = torch.unique(torch.where(top, torch.full_like(m, math.nextafter(1.0 - c, 0.0)), m))
    rows, keep = [], torch.ones_like(m, dtype=torch.bool)
    for n in shapes:
        ok, k = _curve_ranks_vec(c, m, n)
        keep &= ok
        rows.append(k)
    keep &= (m > 0) & ((1.0 - c) - m > 0)
    m, ranks = m[keep], torch.stack(rows)[:, keep]
    for n, row, (K, _) in zip(shapes, ranks, per):
        if not torch.equal(torch.unique(row), K):
            raise RuntimeError(f"tiled_settings: the axis at coarse ratio {c} misses a reachable rank of a shape of {n} patches")
    return m, ranks


class RateCurve(_Rates):
    """rate_curve's result: per image and medium rank K = 0 .. n8 the sizes of the five .bin streams at one coarse ratio.
    nbytes int32 [B,n8+1,5] (0 = not written), bytes int64 [B,n8+1], bpp float64 [B,n8+1], batch_bpp float64 [n8+1];
    ranks: the K a medium ratio reaches (ascending), candidates: the (coarse, medium) pair of each, rank by rank, modes: their
    mode (0, or 1 at coarse ratio 0); n_coarse int64 [B]: coarse patches of each image (ranks up to 4 n_coarse select no medium
    patch).  The curve is not monotone in K: tied patches move together, and a patch that turns medium trades four fine symbols
    for one medium symbol of another length."""

    def __init__(self, nbytes, coarse_ratio, num_pixels, ranks=None, n_coarse=None):
        self.nbytes = nbytes
        self.coarse_ratio = float(coarse_ratio)
        self._set_rates(nbytes, num_pixels, 0, "rate_curve")
        if ranks is None:
            ranks = reachable_ranks((self.bytes.shape[1] - 1) // 4, self.coarse_ratio)
        self.ranks = [int(k) for k, _ in ranks]
        self.candidates = [(self.coarse_ratio, float(m)) for _, m in ranks]
        self.modes = [0 if self.coarse_ratio > 0.0 else 1] * len(self.ranks)
        self.n_coarse = n_coarse

    def ratio(self, K):
        """the (coarse, medium) pair that reaches rank K"""
        return self.candidates[self.ranks.index(int(K))]

    def _choices(self):
        # among the ranks a ratio reaches; choose returns the rank
        sel = torch.tensor(self.ranks, dtype=torch.int64)
        return self.batch_bpp[sel], self.bpp[:, sel], self.ranks.__getitem__


def rate_curve(codec, ind_c, ind_m, ind_f, e16, e8, coarse_ratio, ranks=None):
    """exact sizes of the streams GrainCodec.compress would write for EVERY medium rank at `coarse_ratio`, every image routed on
    its own thresholds on the maps as given (cgic_rate_curve; no threshold-band refinement: maps of
    entropy_maps(x, reference_order=True) make that the reference's routing from the pixels).  The maps may hold any float (NaN,
    +-Inf, negatives, signed zeros, denormals): the sizes are those of the router's masks on them.  Arguments as rate_table's;
    ranks: ((K, medium ratio), ...) to carry instead of reachable_ranks(n16, coarse_ratio).  -> RateCurve"""
    inds, e16c, e8c, (B, h16, w16) = _curve_inputs(ind_c, ind_m, ind_f, e16, e8)
    dev = e16c.device
    n8 = 4 * h16 * w16
    nbytes = torch.empty((B, n8 + 1, _lib.NUM_STREAMS), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(_lib.lib().cgic_rate_curve_workspace_bytes(B, h16, w16)), 16), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("cgic_rate_curve", _table_handle(codec), _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]),
                  _lib.ptr(e16c), _lib.ptr(e8c), B, h16, w16, float(coarse_ratio), _lib.ptr(nbytes), _lib.ptr(ws),
                  _lib.current_stream(dev))
    n_coarse = ws[:B * 16].view(torch.int32).view(B, 4)[:, 0].to(torch.int64).cpu()
    return RateCurve(nbytes, coarse_ratio, 256 * h16 * w16, ranks=ranks, n_coarse=n_coarse)


def _batch_bpp(S, num_pixels, B):
    """RateCurve.batch_bpp's float64 expression for a batch of S bytes"""
    return float(S) * 8 / (int(num_pixels) * max(int(B), 1))


def budget_bytes(target_bpp, num_pixels, B):
    """the largest integer S with float64(S) * 8 / (num_pixels * B) <= target_bpp, in the float64 expression of
    RateCurve.batch_bpp: the byte budget under which an integer comparison S[K] <= budget picks exactly what `choose` picks on
    batch_bpp <= target_bpp.  -1 when not even S = 0 fits (a negative target); capped at 2^62.  Pure host arithmetic"""
    target, P, B = float(target_bpp), int(num_pixels), max(int(B), 1)
    if P <= 0:
        raise ValueError(f"budget_bytes: {num_pixels} pixels")
    if math.isnan(target):
        raise ValueError("budget_bytes: the target is NaN")
    cap = 1 << 62
    if _batch_bpp(cap, P, B) <= target:
        return cap
    if not _batch_bpp(0, P, B) <= target:
        return -1
    S = min(max(int(math.floor(target * (P * B) / 8)), 0), cap)
    while S > 0 and not _batch_bpp(S, P, B) <= target:
        S -= 1
    while S < cap and _batch_bpp(S + 1, P, B) <= target:
        S += 1
    return S


_RANKS_DEV = {}


def _ranks_on_device(dev, n16, c):
    """(K int32 [R] on `dev`, K int64 [R] and medium float64 [R] on the host) of reachable_ranks_vec(n16, c): the ranks
    RateCurve.ranks holds; uploaded once per (device, n16, c)"""
    key = (str(dev), int(n16), float(c))
    hit = _RANKS_DEV.get(key)
    if hit is None:
        K, m = reachable_ranks_vec(int(n16), float(c))
        if len(_RANKS_DEV) >= 64:
            _RANKS_DEV.clear()
        hit = _RANKS_DEV[key] = (K.to(torch.int32).to(dev), K, m)
    return hit


class BppRoute:
    """route_to_bpp's result.  masks: [mask_c, mask_m, mask_f] int32 in the router's layouts, ind int64 [B,h,w], mode: the
    curve's mode (host int: 0, or 1 at coarse ratio 0), choice: the device record int64 [4] = {j, K, fits, batch bytes} (all
    -1 with fits 0 when a requested entry holds a symbol outside the code table; masks and ind are zeros then).
    .rank, .ratio, .fits, .batch_bytes read the record -- the first access synchronises; a captured graph's replays rewrite the
    record: refresh() drops what was read -- and raise KeyError on the -1 record"""

    def __init__(self, masks, ind, mode, choice, coarse_ratio, ranks, mediums):
        self.masks, self.ind, self.mode, self.choice = masks, ind, int(mode), choice
        self.coarse_ratio = float(coarse_ratio)
        self._ranks, self._mediums = ranks, mediums
        self._rec = None

    def refresh(self):
        self._rec = None
        return self

    def _record(self):
        if self._rec is None:
            self._rec = [int(v) for v in self.choice.cpu().tolist()]
        if self._rec[0] < 0:
            raise KeyError("route_to_bpp: an index is not in the code table")
        return self._rec

    @property
    def rank(self):
        return self._record()[1]

    @property
    def ratio(self):
        """the (coarse, medium) pair that reaches the chosen rank"""
        return self.coarse_ratio, float(self._mediums[self._record()[0]])

    @property
    def fits(self):
        return bool(self._record()[2])

    @property
    def batch_bytes(self):
        return self._record()[3]


def route_to_bpp(codec, ind_c, ind_m, ind_f, e16, e8, coarse_ratio, target_bpp=None, budget=None):
    """route a same-size batch at the medium rank whose exact batch bpp is the largest one <= target_bpp, decided ON THE DEVICE
    (cgic_route_to_budget): among the ranks a medium ratio reaches at `coarse_ratio` in the curve's mode (0, or 1 at coarse
    ratio 0; the two ends of the medium axis are other modes: compress_to_bpp(search="curve") covers them), what
    choose(rate_curve(...), target_bpp) picks, then the masks of TripleGrainFixedEntropyRouter(per_image=True) at that rank on
    the maps as given (any float, as rate_curve) and gather_grain_indices of them.  Arguments as rate_curve's.  budget: an int64 device tensor of one
    element, the byte budget of the batch (budget_bytes), used as it is -- a captured graph is replayed with a new target by
    writing into it; else it is made from target_bpp.  The call does not synchronise and copies nothing to the host.
    -> BppRoute"""
    inds, e16c, e8c, (B, h16, w16) = _curve_inputs(ind_c, ind_m, ind_f, e16, e8)
    dev = e16c.device
    c = float(coarse_ratio)
    if (target_bpp is None) == (budget is None):
        raise ValueError("route_to_bpp: give target_bpp or budget (one of them)")
    ranks_dev, ranks, mediums = _ranks_on_device(dev, h16 * w16, c)
    R = int(ranks.numel())
    if R < 1:
        raise ValueError(f"route_to_bpp: no medium ratio reaches a rank at coarse ratio {c}")
    if budget is None:
        budget = torch.full((1,), budget_bytes(target_bpp, 256 * h16 * w16, B), dtype=torch.int64, device=dev)
    elif not (isinstance(budget, torch.Tensor) and budget.dtype == torch.int64 and budget.numel() == 1 and budget.device == dev
              and budget.is_contiguous()):
        raise ValueError("route_to_bpp: budget must be an int64 tensor of one element on the maps' device")
    mc, mm, mf = _lib.grain_masks(B, 4 * h16, 4 * w16, dev)
    ind = torch.empty((B, 4 * h16, 4 * w16), dtype=torch.int64, device=dev)
    choice = torch.empty((4,), dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(_lib.lib().cgic_route_to_budget_workspace_bytes(B, h16, w16, R)), 16), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("cgic_route_to_budget", _table_handle(codec), _lib.ptr(inds[0]), _lib.ptr(inds[1]), _lib.ptr(inds[2]),
                  _lib.ptr(e16c), _lib.ptr(e8c), B, h16, w16, c, _lib.ptr(ranks_dev), R, _lib.ptr(budget), _lib.ptr(mc), _lib.ptr(mm),
                  _lib.ptr(mf), _lib.ptr(ind), _lib.ptr(choice), _lib.ptr(ws), _lib.current_stream(dev))
    return BppRoute([mc, mm, mf], ind, 0 if c > 0.0 else 1, choice, c, ranks, mediums)


def gather_grain_indices(ind_c, ind_m, ind_f, masks):
    """ind [B,h,w] int64 = mask_f ? ind_f : up2(mask_m) ? up2(ind_m) : up4(ind_c) (cgic_gather_grain_indices): the indices of
    the merged latent for these (router) masks"""
    _lib.require_device(ind_c, ind_m, ind_f, *masks)
    mc, mm, mf = (m.contiguous() for m in masks)
    B, h, w = mf.shape[0], mf.shape[-2], mf.shape[-1]
    _lib.require_int32_masks(mc, mm, mf, msg="masks must be int32 like the router's")
    if mc.numel() != B * (h // 4) * (w // 4) or mm.numel() != B * (h // 2) * (w // 2):
        raise ValueError("masks at 1/4, 1/2, 1/1 of the fine grid expected")
    ic, im, if_ = (t.contiguous() for t in (ind_c, ind_m, ind_f))
    if any(t.dtype != torch.int64 for t in (ic, im, if_)) or ic.numel() != mc.numel() or im.numel() != mm.numel() \
            or if_.numel() != mf.numel():
        raise ValueError("grain indices: int64 on the grids of the three masks")
    out = torch.empty((B, h, w), dtype=torch.int64, device=mf.device)
    with _lib.on_device(mf.device):
        _lib.call("cgic_gather_grain_indices", _lib.ptr(ic), _lib.ptr(im), _lib.ptr(if_), _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf),
                  B, h, w, _lib.ptr(out), _lib.current_stream(mf.device))
    return out


class TiledRateCurve(_Rates):
    """rate_curve_tiled's result: per image and setting j of the medium axis the sizes of the five .bin streams, summed over the
    image's tiles, at one coarse ratio.  mediums float64 [M] (ascending), ranks int64 [S, M] (the medium rank of shape class s at
    setting j), shapes [(h16, w16)] per class; nbytes int64 [N, M, 5], bytes int64 [N, M], bpp float64 [N, M] (bits over the
    pixels of the UNPADDED image, inference_high_resolution.py:250,256), batch_bpp float64 [M]; tile_nbytes int32 [T, M, 5] on the
    device, tiles in the order of the groups handed in; tile_shape / tile_image: class and image of each; candidates: the
    (coarse, medium) pair of each setting, modes: their mode.  ends (set by rate_curve_tiled): the two ends of the axis the
    curve's mode does not hold, as an object with candidates, modes, nbytes [2, N, 5], bytes, bpp, batch_bpp"""

    def __init__(self, image_nbytes, tile_nbytes, coarse_ratio, mediums, ranks, shapes, num_pixels, tile_shape=None, tile_image=None):
        self.coarse_ratio = float(coarse_ratio)
        self.mediums = torch.as_tensor(mediums, dtype=torch.float64)
        self.ranks = torch.as_tensor(ranks, dtype=torch.int64)
        self.shapes = list(shapes)
        self.tile_nbytes, self.tile_shape, self.tile_image = tile_nbytes, tile_shape, tile_image
        self.nbytes = image_nbytes.detach().cpu()
        self._set_rates(self.nbytes, num_pixels, 0, "rate_curve_tiled")
        self.candidates = [(self.coarse_ratio, m) for m in self.mediums.tolist()]
        self.modes = [0 if self.coarse_ratio > 0.0 else 1] * len(self.candidates)
        self.ends = None


class _FoldedEnds(RateTable):
    """the ends of a tiled image's medium axis: per-group rate tables folded per image on the host (nbytes int64 [C, N, 5]; their
    entries were checked group by group)"""
    _who = None


def _tile_groups(tiles):
    out = []
    for g in tiles:
        if isinstance(g, dict):
            g = (g["ind_c"], g["ind_m"], g["ind_f"], g["e16"], g["e8"], g["images"])
        ind_c, ind_m, ind_f, e16, e8, images = g
        inds, e16c, e8c, (B, h16, w16) = _curve_inputs(ind_c, ind_m, ind_f, e16, e8)
        images = [int(i) for i in images]
        if len(images) != B or (images and min(images) < 0):
            raise ValueError(f"a group of {B} tiles names the image of {len(images)}")
        out.append((inds, e16c, e8c, images, (h16, w16)))
    return out


def rate_curve_tiled(codec, tiles, coarse_ratio, image_hw=None, settings=None, ends=True):
    """exact sizes of the streams of N tiled images for EVERY setting of the medium ratio at `coarse_ratio`: ONE ratio pair for
    all tiles, every tile routed on its own thresholds on the maps as given, any float in them (the reference's tiling driver,
    inference_high_resolution.py:236-251; maps of entropy_maps(tiles, reference_order=True) make that its routing from the pixels).
    tiles: one entry per shape group, (ind_c, ind_m, ind_f, e16, e8, images) -- or a dict with those keys --: the group's
    grain_indices and maps ([B_g, ...], as rate_curve takes them) and the image index of each of its tiles.  image_hw: the
    (H, W) of the unpadded images for the bpp (default: the pixels of an image's tiles); settings: tiled_settings(...) of the
    groups' shapes in their order, when the caller has it already; ends=False skips the two rate tables per group of the axis' ends.
    One cgic_rate_curve_tiles call for all tiles of all groups.  -> TiledRateCurve"""
    groups = _tile_groups(tiles)
    if not groups:
        raise ValueError("rate_curve_tiled: no tile group")
    c = float(coarse_ratio)
    dev = groups[0][1].device
    shapes = []
    for g in groups:
        if g[4] not in shapes:
            shapes.append(g[4])
    mediums, ranks = settings if settings is not None else tiled_settings([h * w for h, w in shapes], c)
    mediums, ranks = torch.as_tensor(mediums, dtype=torch.float64), torch.as_tensor(ranks, dtype=torch.int64)
    S, M = len(shapes), int(mediums.numel())
    if tuple(ranks.shape) != (S, M) or M < 1:
        raise ValueError(f"rate_curve_tiled: ranks {tuple(ranks.shape)} for {S} shapes and {M} settings")
    for (h, w), row in zip(shapes, ranks):
        if int(row.min()) < 0 or int(row.max()) > 4 * h * w:
            raise ValueError(f"rate_curve_tiled: a rank outside 0 .. {4 * h * w} for tiles of {16 * h}x{16 * w}")
    N = max(max(g[3]) for g in groups if g[3]) + 1
    T = sum(len(g[3]) for g in groups)
    desc = (_lib.RateTile * max(T, 1))()
    off = [0, 0, 0, 0, 0]
    tile_shape, tile_image, pixels = [], [], [0] * N
    t = 0
    for inds, e16c, e8c, images, (h16, w16) in groups:
        n16 = h16 * w16
        k_c = round(n16 * c) if c > 0.0 else 0                          # (cgic_rate_curve's expression: round-half-even of the float64 product)
        s = shapes.index((h16, w16))
        for k, n in enumerate(images):
            desc[t] = _lib.RateTile(h16, w16, k_c, s, n, 0, off[0] + k * n16, off[1] + 4 * k * n16, off[2] + 16 * k * n16,
                                    off[3] + k * n16, off[4] + 4 * k * n16)
            tile_shape.append(s)
            tile_image.append(n)
            pixels[n] += 256 * n16
            t += 1
        B = len(images)
        for i, per in enumerate((n16, 4 * n16, 16 * n16, n16, 4 * n16)):
            off[i] += B * per
    if image_hw is None:
        if len(set(pixels)) != 1:
            raise ValueError("rate_curve_tiled: the images differ in size; give image_hw")
        num_pixels = pixels[0]
    else:
        num_pixels = int(image_hw[0]) * int(image_hw[1])
    cat = lambda i: groups[0][i].reshape(-1) if len(groups) == 1 else torch.cat([g[i].reshape(-1) for g in groups])
    bufs = [groups[0][0][i].reshape(-1) if len(groups) == 1 else torch.cat([g[0][i].reshape(-1) for g in groups]) for i in range(3)]
    bufs += [cat(1), cat(2)]
    count = (ctypes.c_int64 * 5)(*[int(b.numel()) for b in bufs])
    desc_dev = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(dev)
    ranks_dev = ranks.to(torch.int32).contiguous().to(dev)
    image_nbytes = torch.empty((N, M, _lib.NUM_STREAMS), dtype=torch.int64, device=dev)
    tile_nbytes = torch.empty((T, M, _lib.NUM_STREAMS), dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(_lib.lib().cgic_rate_curve_tiles_workspace_bytes(max(T, 1), M, 1)), 16), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("cgic_rate_curve_tiles", _table_handle(codec), *[_lib.ptr(b) for b in bufs], count, desc, _lib.ptr(desc_dev),
                  T, N, c, _lib.ptr(ranks_dev), S, M, _lib.ptr(image_nbytes), _lib.ptr(tile_nbytes), _lib.ptr(ws),
                  _lib.current_stream(dev))
    curve = TiledRateCurve(image_nbytes, tile_nbytes, c, mediums, ranks, shapes, num_pixels, tile_shape, tile_image)
    curve.n_coarse = ws[:T * 16].view(torch.int32).view(T, 4)[:, 0].to(torch.int64).cpu()
    if ends:
        # medium 0 and fine 0: one two-candidate rate table per shape group, folded per image on the host
        cand = _curve_ends(c)
        folded = torch.zeros((len(cand), N, _lib.NUM_STREAMS), dtype=torch.int64)
        for inds, e16c, e8c, images, _ in groups:
            nb = rate_table(codec, *inds, e16c, e8c, cand, per_image=True).nbytes.cpu().to(torch.int64)
            folded.index_add_(1, torch.tensor(images, dtype=torch.int64), nb)
        curve.ends = _FoldedEnds(folded, cand, num_pixels)
    return curve


def _pick_with_ends(curve, target_bpp):
    """_pick over the entries of a curve (RateCurve: the ranks a ratio reaches, TiledRateCurve: its settings) and the two ends of
    its axis (curve.ends) -> (index into cand, fits, cand = curve.candidates + curve.ends.candidates)"""
    ends = getattr(curve, "ends", None)
    cand = curve.candidates + (ends.candidates if ends is not None else [])
    bb = curve._choices()[0].tolist() + (ends.batch_bpp.tolist() if ends is not None else [])
    return (*_pick(bb, cand, float(target_bpp)), cand)


def _encode_captured(model, x, entropy=False):
    """one model.encode(x) with per-image routing forced in the router config and forward hooks on the three encoder heads
    (entropy=True: on the two entropy modules as well); config and hooks are restored whatever encode does
    -> {"c", "m", "f"[, "e8", "e16"]: that module's output}"""
    enc = model.encoder
    params = enc.router_config["params"]
    mods = {"c": enc.conv_out_coarse, "m": enc.conv_out, "f": enc.conv_out_fine}
    if entropy:
        mods.update(e8=model.entropy_calculation_p8, e16=model.entropy_calculation_p16)
    got = {}
    hooks = [mod.register_forward_hook(lambda mod, args, out, name=name: got.__setitem__(name, out)) for name, mod in mods.items()]
    try:
        with routing_per_image(params), torch.no_grad():
            model.encode(x)
    finally:
        for hk in hooks:
            hk.remove()
    return got


def compress_tiled_to_bpp(model, x, target_bpp, tile=None, decode=None):
    """compress tiled high-resolution images at the ONE granularity ratio -- for all images and all tiles, the reference's
    semantics -- whose exact bpp over the batch is the largest one <= target_bpp, among every medium ratio at the router
    config's coarse ratio and the two ends of the axis.  x: one [1,3,H,W] image or N of one size.
    -> (TiledImage, or a list of N; bpp (a list for N > 1): the curve's entry of the chosen setting; (coarse, medium);
    TiledRateCurve with .fits, .chosen (the setting's index, None: an end was chosen)).
    Pad and cut as compress_tiled; per shape group ONE model.encode (the encoder heads are taken from it by forward hooks), the
    maps of entropy_maps(tiles, reference_order=True), grain_indices; one rate_curve_tiled over all groups; then every group
    is routed (per tile, on the maps as given), gathered and compressed at the chosen pair.  decode: None, or
    decode(z_q, masks) -> pixels: then [N,3,H,W] reconstructions are returned as .decoded of each TiledImage
    (decompress_tiled).  Does not touch the usage counter."""
    from . import highres
    from .entropy import entropy_maps
    from .model import _codec_for
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"compress_tiled_to_bpp takes [N,3,H,W], got {tuple(x.shape)}")
    q = model.quantize
    if q.training:
        raise RuntimeError("compress_tiled_to_bpp: the quantiser is in training mode; call model.eval() first")
    tile = highres.TILE if tile is None else int(tile)
    coarse = float(model.encoder.router_config["params"]["coarse_grain_ratio"])
    codec = _codec_for(model)
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    pad, grid, order, batches = highres.cut_groups(x, tile)
    groups = []
    with torch.no_grad():
        for (_, idxs), batch in zip(order, batches):
            got = _encode_captured(model, batch)
            inds = grain_indices(q, got["c"], got["m"], got["f"], getattr(model, "quant_conv", None))
            e8, e16 = entropy_maps(batch, reference_order=True)
            groups.append((*inds, e16, e8, [n for n in range(N) for _ in idxs]))
        curve = rate_curve_tiled(codec, groups, coarse, image_hw=(H, W))
        c, fits, cand = _pick_with_ends(curve, target_bpp)
        cr, mr = cand[c]
        M = len(curve.candidates)
        curve.fits, curve.chosen = fits, (c if c < M else None)
        router = TripleGrainFixedEntropyRouter(cr, mr, per_image=True)
        comp_groups = []
        for (_, idxs), (ind_c, ind_m, ind_f, e16, e8, _) in zip(order, groups):
            masks, _, _, mode = router(e16, e8, want_gate=False)
            ind = gather_grain_indices(ind_c, ind_m, ind_f, masks)
            comp_groups.append((idxs, codec.compress(ind, masks, mode), (ind.reshape(-1), masks, mode)))
        out = highres.assemble_tiled((H, W), pad, grid, comp_groups, N)
        if decode is not None:
            for t in out:
                t.decoded = highres.decompress_tiled(t, codec, decode=decode)[1]
    bpp = (curve.bpp[:, c] if c < M else curve.ends.bpp[c - M]).tolist()
    if N == 1:
        return out[0], bpp[0], (cr, mr), curve
    return out, bpp, (cr, mr), curve


def _pick(bpp, candidates, target):
    """index of the largest bpp <= target (ties: smaller coarse, then smaller medium); none fits: the smallest bpp"""
    idx = list(range(len(candidates)))
    fit = [i for i in idx if bpp[i] <= target]
    if fit:
        return min(fit, key=lambda i: (-bpp[i], candidates[i][0], candidates[i][1])), True
    return min(idx, key=lambda i: (bpp[i], candidates[i][0], candidates[i][1])), False


def choose(table, target_bpp, per="batch"):
    """the candidate with the largest bpp that is <= target_bpp (ties: the smaller coarse ratio, then the smaller medium ratio);
    if none fits, the smallest-bpp candidate with fits=False.  per="batch": on batch_bpp -> (c, fits); per="image": on each
    image's bpp -> (c [B] int64, fits [B] bool) numpy-free lists as tensors, for callers that compress image by image.
    table: a RateTable (c = the candidate's index), a RateCurve (c = the medium rank K, among the ranks a ratio reaches; the
    curve is not monotone in K, so this is a search over all of them, not a bisection) or a TiledRateCurve (c = the index of
    the setting on its medium axis)"""
    target = float(target_bpp)
    if not table.candidates:
        raise ValueError("choose: no candidate (a curve: no medium ratio reaches a rank at its coarse ratio)")
    batch_bpp, image_bpp, value = table._choices()
    if per == "batch":
        c, f = _pick(batch_bpp.tolist(), table.candidates, target)
        return value(c), f
    if per == "image":
        picks = [_pick(row.tolist(), table.candidates, target) for row in image_bpp]
        return torch.tensor([value(c) for c, _ in picks], dtype=torch.int64), torch.tensor([f for _, f in picks], dtype=torch.bool)
    raise ValueError(f"choose: per={per!r}; 'batch' or 'image'")


def _curve_ends(coarse_ratio):
    """the two ends of the medium axis the curve's mode does not hold: medium 0 and fine 0 (modes 2 and 3; coarse 0: 6 and 5)"""
    c = float(coarse_ratio)
    return [(c, 0.0)] if c == 1.0 else [(c, 0.0), (c, 1.0 - c)]


def compress_to_bpp(model, input, target_bpp, candidates=None, decode=True, search="candidates"):
    """compress a batch at the granularity ratio whose exact bpp over the batch is the largest one <= target_bpp.
    -> (dec [B,3,H,W] or None, bpp list[B], CompressedBatch, (coarse, medium), RateTable).
    One model.encode (the three encoder heads and the entropy maps are taken from it by forward hooks), one rate table over the
    candidates (default: default_candidates(the router config's coarse ratio)), then the chosen ratio is routed, gathered,
    compressed and decoded exactly as compress_batch does (per-image routing): bit-identical to compress_batch with the router
    config set to that ratio.  Does not touch the usage counter.
    search="curve": instead of the candidates, EVERY medium ratio at the router config's coarse ratio -- one rate_curve over all
    medium ranks plus the two ends of the axis (medium 0, fine 0) from a rate table, on the maps of
    entropy_maps(input, reference_order=True), on which routing on the maps as given is the reference's routing from the pixels.
    Returns a RateCurve in place of the table, with .fits, .chosen_rank (None: an end was chosen) and .ends (their RateTable);
    the returned bpp is the curve's entry of the chosen rank.
    search="device": the curve search with the decision kept on the GPU (route_to_bpp): on the same maps, the curve at every
    rank a medium ratio reaches, the pick, the masks and the merged indices in one launch chain without a host synchronisation;
    the host reads the choice only after the coder has been enqueued.  It covers the INTERIOR of the medium axis only -- the
    curve's mode, medium > 0 and fine > 0: the two ends are other routing modes, and which streams a mode writes is a host
    argument of the coder; search="curve" remains the way to include them.  Returns the BppRoute in place of the table (.rank,
    .ratio, .fits, .batch_bytes); KeyError if an index is not in the code table."""
    from .model import _codec_for, _decode
    assert len(input.shape) == 4
    if search not in ("candidates", "curve", "device"):
        raise ValueError(f"compress_to_bpp: search={search!r}; 'candidates', 'curve' or 'device'")
    if search != "candidates" and candidates is not None:
        raise ValueError(f"compress_to_bpp: search={search!r} takes no candidates (it covers every medium ratio of the router config's coarse ratio)")
    q = model.quantize
    if q.training:
        raise RuntimeError("compress_to_bpp: the quantiser is in training mode; call model.eval() first")
    params = model.encoder.router_config["params"]
    if search == "candidates":
        if candidates is None:
            candidates = default_candidates(params["coarse_grain_ratio"])
        cand = _check_candidates(candidates)
    codec = _codec_for(model)
    got = _encode_captured(model, input, entropy=search == "candidates")
    with torch.no_grad():
        ind_c, ind_m, ind_f = grain_indices(q, got["c"], got["m"], got["f"], getattr(model, "quant_conv", None))
        if search == "device":
            from .entropy import entropy_maps
            e8, e16 = entropy_maps(input, reference_order=True)
            route = route_to_bpp(codec, ind_c, ind_m, ind_f, e16, e8, float(params["coarse_grain_ratio"]), target_bpp=target_bpp)
            comp = codec.compress(route.ind, route.masks, route.mode)
            ratio = route.ratio                                          # (the first read of the choice: KeyError on the -1 record)
            bpp = comp.bpp(input.shape[2] * input.shape[3])
            dec = _decode(model, codec, comp) if decode else None
            return dec, bpp, comp, ratio, route
        if search == "curve":
            from .entropy import entropy_maps
            coarse = float(params["coarse_grain_ratio"])
            e8, e16 = entropy_maps(input, reference_order=True)
            table = rate_curve(codec, ind_c, ind_m, ind_f, e16, e8, coarse)
            table.ends = rate_table(codec, ind_c, ind_m, ind_f, e16, e8, _curve_ends(coarse), per_image=True)
            c, fits, cand = _pick_with_ends(table, target_bpp)
            table.chosen_rank = table.ranks[c] if c < len(table.ranks) else None
        else:
            e16, e8 = got["e16"], got["e8"]
            table = rate_table(codec, ind_c, ind_m, ind_f, e16, e8, cand, per_image=True)
            c, fits = choose(table, target_bpp)
        cr, mr = cand[c]
        router = TripleGrainFixedEntropyRouter(cr, mr, per_image=True)
        masks, _, _, mode = router(e16, e8, want_gate=False)
        ind = gather_grain_indices(ind_c, ind_m, ind_f, masks)
        comp = codec.compress(ind, masks, mode)
        bpp = comp.bpp(input.shape[2] * input.shape[3])
        dec = _decode(model, codec, comp) if decode else None
    table.fits = fits
    return dec, bpp, comp, (cr, mr), table
