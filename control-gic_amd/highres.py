"""Tiling driver for high-resolution images -- the hot-path side of inference_high_resolution.py.

The reference pads the image to a multiple of 16 (centred zero pad, :145-173,:227-228), cuts it into a
non-overlapping 768-px grid with ragged last row/column (:112-125) and calls `model.compress` once per tile
at B=1 (:246), overwriting the same five .bin files every time; bpp is accumulated as
sum(bpp_tile * tile_w * tile_h) / (W * H) of the UNPADDED image (:250,:256).

Here tiles of equal shape are batched through the kernels together (router thresholds stay per tile =
per image of the batch), the streams stay on the device, and the accounting is the reference's.
"""
import ctypes
import math

import torch

from . import _lib
from .codec import GrainCodec
from .pipeline import image_io_buffers

TILE = 768


def compute_padding(in_h, in_w, min_div=16):
    """(left, right, top, bottom) pad and the matching unpad -- inference_high_resolution.py:145-173"""
    out_h = (in_h + min_div - 1) // min_div * min_div
    out_w = (in_w + min_div - 1) // min_div * min_div
    left = (out_w - in_w) // 2
    right = out_w - in_w - left
    top = (out_h - in_h) // 2
    bottom = out_h - in_h - top
    return (left, right, top, bottom), (-left, -right, -top, -bottom)


def center_crop16(x, div=16):
    """[..., H, W] -> the centred [..., div*(H//div), div*(W//div)] window: the dataset transform of both reference scripts
    (`_resize_and_crop`, inference.py:62-68 = inference_high_resolution.py:62-68: torchvision's center_crop, whose offsets are
    int(round((H - H') / 2.0)) with Python's round-half-to-even).  A view, no copy"""
    H, W = x.shape[-2:]
    th, tw = div * (H // div), div * (W // div)
    top, left = int(round((H - th) / 2.0)), int(round((W - tw) / 2.0))
    return x[..., top:top + th, left:left + tw]


def tile_grid(h, w, tile=TILE):
    """row-major list of (y, x, tile_h, tile_w) -- nonoverlapping_grid_indices, :112-125 + the loop at :236-244"""
    ys = list(range(0, h, tile))
    xs = list(range(0, w, tile))
    ths = [tile] * (h // tile) + ([h % tile] if h % tile else [])
    tws = [tile] * (w // tile) + ([w % tile] if w % tile else [])
    return [(y, x, th, tw) for y, th in zip(ys, ths) for x, tw in zip(xs, tws)]


def gaussian_weights(tile_width, tile_height, device=None):
    """[1,3,tile_h,tile_w] float64 blend weights -- _gaussian_weights, :127-143 (note the reference's
    asymmetric midpoints: (w-1)/2 for x, h/2 for y)"""
    var = 0.01
    mx = (tile_width - 1) / 2
    xp = [math.exp(-(x - mx) * (x - mx) / (tile_width * tile_width) / (2 * var)) / math.sqrt(2 * math.pi * var)
          for x in range(tile_width)]
    my = tile_height / 2
    yp = [math.exp(-(y - my) * (y - my) / (tile_height * tile_height) / (2 * var)) / math.sqrt(2 * math.pi * var)
          for y in range(tile_height)]
    wts = torch.tensor(yp, dtype=torch.float64)[:, None] * torch.tensor(xp, dtype=torch.float64)[None, :]
    return wts.to(device).expand(1, 3, tile_height, tile_width)


_factors = {}            # (device, n, axis) -> float64 [n]: the one-dimensional factors of gaussian_weights, made by the library


def tile_weight_factors(n, axis, device=None):
    """float64 [n]: the one-dimensional factors of gaussian_weights from the library (cgic_tile_weights_host) -- axis 0 = x
    (midpoint (n-1)/2), axis 1 = y (midpoint n/2): gaussian_weights(tw, th)[0, 0] == outer(factors(th, 1), factors(tw, 0)), bit for
    bit.  device None / "cpu": a host tensor; a HIP device: uploaded once and cached per (device, n, axis).  The first upload is a
    host-to-device copy and must happen OUTSIDE a graph capture (TiledCall makes its factors when it is built; otherwise call this,
    or paste once eagerly, before capturing)"""
    dev = torch.device("cpu" if device is None else device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev, int(n), int(axis))
    t = _factors.get(key)
    if t is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"tile_weight_factors({n}, {axis}): the factors of this tile extent are not on {dev} yet and a stream is being "
                               "captured -- their first upload is a host-to-device copy and must happen outside a graph capture (paste once "
                               "eagerly, or call tile_weight_factors for every tile extent, before capturing)")
        host = (ctypes.c_double * int(n))() if n >= 1 else None
        _lib.call("cgic_tile_weights_host", int(n), int(axis), host)
        t = torch.tensor(list(host), dtype=torch.float64).to(dev)
        _factors[key] = t
    return t


def _shape_groups(tiles):
    """the shape groups [((th, tw), tile indices)] of a tile grid, largest first (the order of cut_groups / compress_tiled_batch)"""
    by_shape = {}
    for i, (_, _, th, tw) in enumerate(tiles):
        by_shape.setdefault((th, tw), []).append(i)
    return sorted(by_shape.items(), key=lambda kv: -len(kv[1]) * kv[0][0] * kv[0][1])


def tile_geometry(H, W, tile=TILE):
    """the tiling of an unpadded HxW image -> (pad, tiles, groups): the centred pad (left, right, top, bottom) to multiples of 16, the
    row-major tile grid of the padded image and its shape groups, largest first.  Bytes, pictures and bpp all follow this order"""
    pad, _ = compute_padding(H, W)
    left, right, top, bottom = pad
    tiles = tile_grid(H + top + bottom, W + left + right, tile)
    return pad, tiles, _shape_groups(tiles)


def _check_groups(tiles, groups, what):
    if sorted(i for _, idxs in groups for i in idxs) != list(range(len(tiles))) or \
            any(tuple(tiles[i][2:]) != tuple(shape) for shape, idxs in groups for i in idxs):
        raise ValueError(f"{what}: groups must name every tile once, under its own shape")


def _resolve_geometry(H, W, tile, tiles, groups, what, cover=True):
    """(top, left, tiles, groups) of an unpadded HxW image: what tile_geometry derives from `tile`, or the caller's own tiles / groups,
    checked"""
    (left, _, top, _), grid, order = tile_geometry(H, W, tile)
    if tiles is None:
        tiles = grid
    else:
        _check_cover(H, W, top, left, tiles, what, cover)
    if groups is None:
        groups = order if tiles is grid else _shape_groups(tiles)
    else:
        _check_groups(tiles, groups, what)
    return top, left, tiles, groups


def _placed(tiles, groups, top, left):
    """the tiles in launch order, shape group by shape group -> (group, position in the group, group size T, y0, x0, th, tw) with the
    origin in UNPADDED coordinates (negative inside the pad): what a tile descriptor of the library is built from.  In an image-major
    batch [N * T, ...] the tile sits `position` tiles behind image 0's first and T tiles before the next image's"""
    for g, ((th, tw), idxs) in enumerate(groups):
        for k, i in enumerate(idxs):
            yield g, k, len(idxs), tiles[i][0] - top, tiles[i][1] - left, th, tw


def _check_cover(H, W, top, left, tiles, what="paste_tiles", cover=True):
    """every pixel of the unpadded image belongs to exactly one tile (the closed form of cgic_paste_tiles holds for such grids only)"""
    clipped = []
    for (y, x, th, tw) in tiles:
        y0, y1, x0, x1 = max(y - top, 0), min(y - top + th, H), max(x - left, 0), min(x - left + tw, W)
        if y0 < y1 and x0 < x1:
            clipped.append((y0, y1, x0, x1))
    for k, (y0, y1, x0, x1) in enumerate(clipped):
        for (v0, v1, u0, u1) in clipped[:k]:
            if not (y1 <= v0 or v1 <= y0 or x1 <= u0 or u1 <= x0):
                raise ValueError(f"{what}: tiles overlap (the reference's grid never does: inference_high_resolution.py:112-125)")
    if cover and sum((y1 - y0) * (x1 - x0) for y0, y1, x0, x1 in clipped) != H * W:
        raise ValueError(f"{what}: the tile grid does not cover the {H}x{W} image (a pixel without a tile would be left unwritten)")


def _paste(pixels, H, W, top, left, tiles, groups, N, weighted, frames, out):
    if torch.is_tensor(pixels):
        pixels = [pixels]
    if len(pixels) != len(groups):
        raise ValueError(f"paste_tiles: {len(pixels)} tile batches for {len(groups)} shape groups")
    for ((th, tw), idxs), b in zip(groups, pixels):
        if tuple(b.shape) != (N * len(idxs), 3, th, tw) or b.dtype != torch.float32 or not b.is_contiguous():
            raise ValueError(f"paste_tiles: the batch of the {th}x{tw} tiles must be contiguous fp32 [{N * len(idxs)},3,{th},{tw}] (image-major), "
                             f"got {b.dtype} {tuple(b.shape)}")
        if tw % 4:
            raise ValueError(f"paste_tiles: tile width {tw} is not a multiple of 4")
    _lib.require_device(*pixels)
    dev = pixels[0].device
    if any(b.device != dev for b in pixels):
        raise ValueError("paste_tiles: the tile batches live on different devices")
    want, dt = ((N, H, W, 3), torch.uint8) if frames else ((N, 3, H, W), torch.float32)
    if out is None:
        out = torch.empty(want, dtype=dt, device=dev)
    elif tuple(out.shape) != want or out.dtype != dt or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"paste_tiles: out must be contiguous {dt} {list(want)} on {dev}")
    wts = [(tile_weight_factors(tw, 0, dev).data_ptr(), tile_weight_factors(th, 1, dev).data_ptr()) if weighted else (None, None)
           for (th, tw), _ in groups]
    desc = [_lib.PasteTile(pixels[g].data_ptr() + k * 3 * th * tw * 4, T * 3 * th * tw, wts[g][0], wts[g][1], y0, x0, th, tw)
            for g, k, T, y0, x0, th, tw in _placed(tiles, groups, top, left)]
    with torch.cuda.device(dev):
        stream = _lib.current_stream(dev)
        for at in range(0, len(desc), 96):                       # (cgic_paste_tiles takes 96 tiles a launch)
            part = desc[at:at + 96]
            _lib.call("cgic_paste_tiles", N, H, W, len(part), (_lib.PasteTile * len(part))(*part),
                      None if frames else out.data_ptr(), out.data_ptr() if frames else None, stream)
    return out


def paste_tiles(pixels, hw, tiles=None, groups=None, N=1, weighted=True, frames=False, out=None, tile=TILE):
    """the way out of the tiling driver -- blend, normalise, clamp, unpad (inference_high_resolution.py:231-255) and with frames=True
    the uint8 conversion of write_images (:103) -- as ONE launch for all tiles of all N images (cgic_paste_tiles), bit-identical to
    the reference's loop on the CPU.
    pixels: per shape group one fp32 batch [N*T,3,th,tw], image-major (the layout of cut_groups / compress_tiled_batch: what a decoder
    called once per group returns); hw = (H, W) of the unpadded image.  tiles (row-major (y, x, th, tw) in padded coordinates) and
    groups ([((th, tw), tile indices)]) default to what cut_groups derives from hw and `tile`; given, the grid must cover the image.
    weighted=False: no blend weights, the result is clamp(p, 0, 1) (what the loop would give if its weights cancelled exactly).
    -> [N,3,H,W] fp32, or uint8 frames [N,H,W,3].  With `out` (that shape, contiguous) nothing is allocated and nothing synchronises:
    capturable, once the weight factors of the tile extents are on the device (tile_weight_factors).  More than 96 tiles are several launches."""
    H, W = int(hw[0]), int(hw[1])
    top, left, tiles, groups = _resolve_geometry(H, W, tile, tiles, groups, "paste_tiles")
    return _paste(pixels, H, W, top, left, tiles, groups, int(N), weighted, frames, out)


def _partition(x, H, W, top, left, tiles, groups, masks, N, frames, out):
    """cgic_partition_map for the tiles of N images: masks = per shape group (mask_c, mask_m, mask_f), each the image-major buffer of
    the group's N * T tiles, read in place"""
    from . import draw
    if len(masks) != len(groups):
        raise ValueError(f"partition_tiles: masks of {len(masks)} shape groups for {len(groups)}")
    trios = []
    for ((th, tw), idxs), m in zip(groups, masks):
        T = len(idxs)
        if th % 16 or tw % 16:
            raise ValueError(f"partition_tiles: tile {th}x{tw}: the router's masks belong to tiles whose sides are multiples of 16")
        m = list(m)
        if len(m) != 3:
            raise ValueError("partition_tiles: per shape group the router's three masks (coarse, medium, fine)")
        _lib.require_device(*m)
        _lib.require_int32_masks(*m)
        for t, d in zip(m, (16, 8, 4)):
            if t.numel() != N * T * (th // d) * (tw // d) or tuple(t.shape[-2:]) != (th // d, tw // d) or not t.is_contiguous() or t.device != x.device:
                raise ValueError(f"partition_tiles: a mask of the {th}x{tw} tiles must be contiguous int32 [{N * T},1,{th // d},{tw // d}] (image-major) "
                                 f"on {x.device}, got {tuple(t.shape)}")
        trios.append(m)
    desc = [_lib.PartitionTile(*[_lib.ptr(t) + k * (th // d) * (tw // d) * 4 for t, d in zip(trios[g], (16, 8, 4))], None, T, y0, x0, th, tw, 0, 0)
            for g, k, T, y0, x0, th, tw in _placed(tiles, groups, top, left)]
    return draw._launch(x, N, H, W, desc, frames, out, "partition_tiles")


def _group_masks(tiled_list):
    """per shape group the image-major mask buffers behind a list of TiledImages of one geometry: the shared buffers themselves where
    the images are views of them one after the other (compress_tiled_batch, TiledCall), a concatenation otherwise"""
    first = tiled_list[0]
    for t in tiled_list[1:]:
        if t.tiles != first.tiles or t.image_hw != first.image_hw or [g[0] for g in t.groups] != [g[0] for g in first.groups]:
            raise ValueError("partition_tiles: the images differ in geometry")
    out = []
    for lane in range(len(first.groups)):
        per = [t.groups[lane][2][1] for t in tiled_list]                  # per image: [mask_c, mask_m, mask_f] of its T tiles
        trio = []
        for j in range(3):
            ms = [p[j] for p in per]
            step = ms[0].numel() * ms[0].element_size()
            store = ms[0].untyped_storage().data_ptr()
            in_place = all(m.is_contiguous() and m.shape == ms[0].shape and m.untyped_storage().data_ptr() == store
                           and m.data_ptr() == ms[0].data_ptr() + n * step for n, m in enumerate(ms))
            if in_place:                                         # N consecutive views of one buffer: that buffer, as one view
                base = ms[0]
                trio.append(base.as_strided((len(ms) * base.shape[0],) + tuple(base.shape[1:]), base.stride(), base.storage_offset()))
            else:
                trio.append(torch.cat([m.contiguous() for m in ms]))
        out.append(trio)
    return out


def partition_tiles(x, tiled, frames=False, out=None, tile=TILE, tiles=None, groups=None):
    """the partition map of tiled images -- the picture inference_high_resolution.py's -w promises (:188-189) and never draws (it passes
    False at :246) -- as ONE launch for all tiles of all N images (cgic_partition_map).  Defined as: per tile, the reference's
    draw_triple_grain_256res (CGIC/modules/draw.py:78-119) on that tile of the PADDED image with that tile's grain indices, then the
    unpad of :255; tiles never overlap, so that is well defined.
    x: the unpadded images, fp32 [N,3,H,W] or uint8 frames [N,H,W,3].  tiled: a TiledImage (N = 1), the list of N from
    compress_tiled_batch / TiledCall (their shared per-group mask buffers are read in place), or -- with the geometry from `tile`, or
    from tiles= / groups= as paste_tiles takes them -- per shape group the router's three masks [N*T,1,..] (image-major).
    -> fp32 [N,3,H,W] (line pixels -1), or with frames=True uint8 frames [N,H,W,3] (line pixels 1); x is not modified unless `out is x`.
    With `out` nothing is allocated and nothing synchronises.  More than 84 tiles are several launches."""
    from . import draw
    _lib.require_device(x)
    _, N, H, W = draw._image_shape(x, "partition_tiles")
    if not x.is_contiguous():
        if out is x:
            raise ValueError("partition_tiles: an in-place draw needs a contiguous image")
        x = x.contiguous()
    if isinstance(tiled, TiledImage):
        tiled = [tiled]
    if len(tiled) and isinstance(tiled[0], TiledImage):
        first = tiled[0]
        if tuple(first.image_hw) != (H, W) or len(tiled) != N:
            raise ValueError(f"partition_tiles: {len(tiled)} tiled images of {tuple(first.image_hw)} for x {tuple(x.shape)}")
        (left, _, top, _), _ = compute_padding(H, W)
        tiles, groups, masks = first.tiles, first.shape_groups(), _group_masks(tiled)
    else:
        # the caller's tiles: disjoint always (the library checks it per launch only, and more than 84 tiles are several launches); a
        # hole is allowed where the caller's `out` already holds what the uncovered pixels keep
        top, left, tiles, groups = _resolve_geometry(H, W, tile, tiles, groups, "partition_tiles", cover=out is None)
        masks = tiled
    return _partition(x, H, W, top, left, tiles, groups, masks, N, bool(frames), out)


def to_frames(x, out=None):
    """the untiled way out: x [N,3,H,W] fp32 -> uint8 frames [N,H,W,3] = (255 * x.clamp(0, 1).permute(0, 2, 3, 1)).astype(uint8), the
    clamp of inference.py:163 followed by write_images (inference_high_resolution.py:103), as a one-tile unweighted cgic_paste_tiles
    (NaN -> 0).  W must be a multiple of 4 (the reference's inputs are cropped to multiples of 16)"""
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError(f"to_frames takes fp32 [N,3,H,W], got {x.dtype} {tuple(x.shape)}")
    N, _, H, W = x.shape
    if W % 4:
        raise ValueError(f"to_frames: width {W} is not a multiple of 4")
    return _paste([x.contiguous()], H, W, 0, 0, [(0, 0, H, W)], [((H, W), [0])], N, False, True, out)


class TiledImage:
    """result of compress_tiled: per shape-group CompressedBatch + where each tile sits"""

    def __init__(self, image_hw, pad, tiles, groups):
        self.image_hw = image_hw          # (H, W) unpadded
        self.pad = pad                    # (left, right, top, bottom)
        self.tiles = tiles                # [(y, x, th, tw)] row-major, padded coordinates
        self.groups = groups              # [(tile indices, CompressedBatch, encode outputs)]

    def shape_groups(self):
        """[((th, tw), tile indices)] in this image's group order: what paste_tiles / partition_tiles take as groups="""
        return [(tuple(self.tiles[idxs[0]][2:]), idxs) for idxs, _, _ in self.groups]

    def tile_bpp(self):
        bpp = [None] * len(self.tiles)
        for idxs, comp, _ in self.groups:
            for i, v in zip(idxs, comp.bpp()):
                bpp[i] = v
        return bpp

    def bpp(self):
        """bit_sum / (W * H) of the unpadded image -- inference_high_resolution.py:250,256"""
        bits = sum(b * tw * th for b, (_, _, th, tw) in zip(self.tile_bpp(), self.tiles))
        return bits / self.image_hw[1] / self.image_hw[0]

    def pack(self, image_id=0):
        """the container of this image's tiles, built on the device: container.pack_device(self, ...) -> PackedContainer"""
        from .container import pack_device
        return pack_device(self, first_image_id=image_id)

    def streams(self):
        """per tile (row-major) {stream name: bytes}"""
        out = [None] * len(self.tiles)
        for idxs, comp, _ in self.groups:
            for i, s in zip(idxs, comp.to_host()):
                out[i] = s
        return out


# ---- shape groups side by side.  A 2040x1356 image is 6 tiles in 4 shape groups of one or two tiles: each group's launches
# keep a handful of CUs busy, so the groups cost what the slowest one costs when they run on parallel streams (forked from
# and joined back into the caller's stream by events -- which is also what a hipGraph capture of the whole image records).
_side_streams = {}


def _tensors_of(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            yield from _tensors_of(o)
    elif hasattr(obj, "data") and hasattr(obj, "nbytes") and torch.is_tensor(getattr(obj, "data", None)):
        yield obj.data
        yield obj.nbytes


class _Fork:
    """run the bodies of `for k, st in fork.lanes(n)` on n streams: lane 0 is the current stream, the others wait for what was
    queued on it so far; join() makes the current stream wait for all of them and tells the allocator about the hand-over"""

    def __init__(self, device, enabled):
        self.cur = torch.cuda.current_stream(device)
        self.enabled = enabled
        self.used = []
        self.device = device
        # ONE fork point, recorded before lane 0's body is queued: a side lane waits for what precedes the fork, not for the
        # (largest) group that lane 0 runs -- recorded lazily, the side lanes only started once that group was over
        self.fork_ev = None
        if enabled:
            self.fork_ev = torch.cuda.Event()
            self.fork_ev.record(self.cur)

    def on(self, k):
        """context of lane k's stream (no context switch at all when the fork is off: ~10 us of torch per use)"""
        return torch.cuda.stream(self.lane(k)) if self.enabled else _lib._null_ctx

    def lane(self, k):
        if not self.enabled or k == 0:
            return self.cur
        pool = _side_streams.setdefault(torch.device(self.device).index or 0, [])
        while len(pool) < k:
            pool.append(torch.cuda.Stream(self.device))
        st = pool[k - 1]
        if st not in self.used:
            st.wait_event(self.fork_ev)              # everything before the fork
            self.used.append(st)
        return st

    def join(self, produced=()):
        for st in self.used:
            ev = torch.cuda.Event()
            ev.record(st)
            self.cur.wait_event(ev)
        if self.used:
            for t in _tensors_of(list(produced)):
                t.record_stream(self.cur)            # allocated on a side stream, consumed (and eventually freed) on this one
        self.used = []


def _cut_all(x, frames, N, H, W, top, left, tiles, order):
    """the tile batches of all shape groups from the unpadded image(s) in one launch -> [batch per group], batch
    [N, T, 3, th, tw] fp32 or [N, T, th, tw, 3] uint8 (inference_high_resolution.py:145-173 pad + :236-244 crop)"""
    _lib.require_device(x)
    batches = [torch.empty((N, len(idxs), th, tw, 3) if frames else (N, len(idxs), 3, th, tw), dtype=x.dtype, device=x.device)
               for (th, tw), idxs in order]
    desc = [_lib.Tile(batches[g].data_ptr() + k * 3 * th * tw * x.element_size(), T * 3 * th * tw, y0, x0, th, tw)
            for g, k, T, y0, x0, th, tw in _placed(tiles, order, top, left)]
    with torch.cuda.device(x.device):
        _lib.call("cgic_cut_tiles", _lib.ptr(x), int(frames), N, H, W, len(desc), (_lib.Tile * len(desc))(*desc), _lib.current_stream(x.device))
    return batches


def _compress_groups(x, encode, codec, tile, concurrent, chain=False, fuse_maps=True, frames_fp32=False):
    """x [N,3,H,W] fp32 -- or uint8 frames [N,H,W,3], the tiles then reach `encode` as uint8 [T,th,tw,3] (entropy_maps_u8 makes the
    fp32 tiles and the maps in one pass) --: the shape groups of N images of one size, each group ONE batch of N * T tiles (image-major)
    -> (H, W), pad, tiles, [(tile indices, CompressedBatch, (ind, masks, mode))]"""
    frames = x.dtype == torch.uint8
    if frames and x.shape[-1] != 3 or not frames and x.shape[1] != 3:
        raise ValueError(f"expected [N,3,H,W] (or uint8 [N,H,W,3]), got {x.dtype} {tuple(x.shape)}")
    N = x.shape[0]
    H, W = (x.shape[1], x.shape[2]) if frames else (x.shape[2], x.shape[3])
    # the largest group first: it is the long pole, and lane 0 (no fork latency) is its stream
    pad, tiles, order = tile_geometry(H, W, tile)
    left, _, top, _ = pad
    groups = []
    chain = chain and 1 < len(order) <= _lib.lib().cgic_group_max()
    fork = _Fork(x.device, concurrent and not chain)
    xv = x.permute(0, 3, 1, 2) if frames else x              # [N,3,H,W] view either way
    # chain: ONE launch chain for all shape groups (cgic_group_begin / _launch): every group's calls are recorded, then issued as
    # one launch per kernel whose grid is the concatenation of the groups' grids
    grp = _lib.launch_group(len(order), [N * len(idxs) * th * tw for (th, tw), idxs in order], x.device) if chain else None
    batches = []
    cut, made = None, []
    if chain and (not frames or frames_fp32) and fuse_maps and max(len(idxs) for _, idxs in order) <= 48:
        # pad + crop + BOTH entropy maps of all shape groups in ONE launch (cgic_entropy_maps_tiles, grouped): the tile batches come
        # back tagged with their maps -- encode's entropy_maps(tiles) returns them without another pass over the pixels
        from .entropy import entropy_maps_tiles
        xc = x.contiguous()
        cut, made = [], []
        with _lib.launch_group(len(order), [N * len(idxs) * th * tw for (th, tw), idxs in order], x.device) as g:
            for k, ((th, tw), idxs) in enumerate(order):
                g.select(k)
                t, e8_, e16_ = entropy_maps_tiles(xc, [(tiles[i][0] - top, tiles[i][1] - left) for i in idxs], th, tw)
                made.append((e8_, e16_, e8_._cgic_flat8))           # (strong references for the length of this call)
                cut.append(t.view(N, len(idxs), 3, th, tw))
    elif not fork.enabled and len(tiles) <= 96:
        # pad + crop of ALL tiles as one launch (cgic_cut_tiles): every tile written straight from the unpadded image
        cut = _cut_all(x.contiguous(), frames, N, H, W, top, left, tiles, order)
    for lane, ((th, tw), idxs) in enumerate(order):
        with fork.on(lane):
            # pad + cut in ONE copy per tile (F.pad of the whole image and a stack of views would move every pixel twice): a tile
            # is the part of the image it covers, zeros where it reaches into the centred pad
            batch = cut[lane] if cut is not None else \
                torch.empty((N, len(idxs), th, tw, 3) if frames else (N, len(idxs), 3, th, tw), dtype=x.dtype, device=x.device)
            bv = batch.permute(0, 1, 4, 2, 3) if frames and not made else batch
            for k, i in enumerate(idxs if cut is None else ()):
                y0, x0 = tiles[i][0] - top, tiles[i][1] - left                  # in unpadded coordinates
                sy0, sy1, sx0, sx1 = max(y0, 0), min(y0 + th, H), max(x0, 0), min(x0 + tw, W)
                dst = bv[:, k]
                dst[:, :, sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = xv[:, :, sy0:sy1, sx0:sx1]
                # only the strips that reach into the pad are zeroed (a few rows / columns, not the whole batch)
                for strip in (dst[:, :, :sy0 - y0], dst[:, :, sy1 - y0:], dst[:, :, :, :sx0 - x0], dst[:, :, :, sx1 - x0:]):
                    if strip.numel():
                        strip.zero_()
            batch = batch.view(-1, th, tw, 3) if frames and not made else batch.view(-1, 3, th, tw)
            if made:                                     # (tags do not survive a view: this is the object `encode` sees)
                from .entropy import _MadeMaps
                e8, e16, flat8 = made[lane]
                batch._cgic_maps = _MadeMaps(batch, e8, e16, flat8)       # (weak: the maps point back at the batch)
                e8._cgic_pixels = e16._cgic_pixels = batch
            if chain:
                batches.append(batch)
                continue
            ind, masks, mode = encode(batch)
            groups.append((idxs, codec.compress(ind, masks, mode), (ind, masks, mode)))
    if chain:
        with grp as g:
            for k, (((th, tw), idxs), batch) in enumerate(zip(order, batches)):
                g.select(k)
                ind, masks, mode = encode(batch)
                groups.append((idxs, codec.compress(ind, masks, mode), (ind, masks, mode)))
    fork.join([(c, e) for _, c, e in groups])
    return (H, W), pad, tiles, groups


def compress_tiled(x, encode, codec, tile=TILE, concurrent=False, chain=False, fuse_maps=True, frames_fp32=False):
    """x [1,3,H,W] on the device; encode(tiles [T,3,th,tw]) -> (ind [T*h*w] int64, masks [3 x int32], mode)
    with per-tile routing (the reference's per-tile B=1 call); codec: GrainCodec.  -> TiledImage.
    concurrent: the shape groups run on parallel streams (same results; see _Fork).
    chain: the shape groups (four for a 2040x1356 image) go through ONE launch chain -- entropy maps, VQ + router, compress: three
    launches for all six tiles instead of three per group (cgic_group_begin / _launch; same bytes).  `encode` is then called
    inside a launch group: it may allocate and call control_gic_amd's entropy_maps / entropy_maps_u8 / vq_forward_route (whose
    launches are recorded and issued when all groups are in), but must not enqueue torch work that READS their outputs --
    a conv encoder that consumes the router's gate cannot run under chain=True.
    fuse_maps (with chain, fp32 input): the tiles are cut AND their entropy maps made in one pass over the image
    (cgic_entropy_maps_tiles); the tile batches `encode` receives carry their maps, entropy_maps(tiles) returns them as they are.
    frames_fp32 (uint8 frames with chain + fuse_maps): `encode` receives the fp32 tiles T.ToTensor() would have produced (tagged with their
    maps) instead of uint8 tiles -- ToTensor, pad, crop and both maps are then one pass over the frames (3 B read + 12 B written per pixel)."""
    if x.dim() != 4 or x.shape[0] != 1:
        raise ValueError("compress_tiled takes one image [1,3,H,W] (or one uint8 frame [1,H,W,3]; the reference script uses batch 1); "
                         "compress_tiled_batch takes several of one size")
    return TiledImage(*_compress_groups(x, encode, codec, tile, concurrent, chain, fuse_maps, frames_fp32))


def compress_tiled_batch(x, encode, codec, tile=TILE, concurrent=False, chain=False, fuse_maps=True, frames_fp32=False):
    """x [N,3,H,W] (or uint8 frames [N,H,W,3]: `encode` then gets uint8 tiles [T,th,tw,3] for entropy_maps_u8 -- a pad of zero
    bytes is the pad of zeros ToTensor would have produced): N images of ONE size (a folder of camera frames, a DIV2K bucket) -> list of N TiledImage, each what
    compress_tiled gives for that image alone (routing is per tile, so batching across images changes no byte).  The tiles
    of equal shape of ALL the images go through the kernels as one batch: a 2040x1356 image alone is four launch chains of one or
    two tiles each (a handful of workgroups per launch); eight images are chains of 8-16 tiles.  The TiledImages hold views
    of the shared per-group buffers"""
    if x.dim() != 4:
        raise ValueError("compress_tiled_batch takes [N,3,H,W] or uint8 [N,H,W,3]")
    N = x.shape[0]
    hw, pad, tiles, groups = _compress_groups(x, encode, codec, tile, concurrent, chain, fuse_maps, frames_fp32)
    return assemble_tiled(hw, pad, tiles, groups, N)


def assemble_tiled(hw, pad, tiles, groups, N, whole=True):
    """the N TiledImages of shape groups that hold the tiles of N images of one size image-major ([N * T, ...] per group:
    (tile indices, CompressedBatch, (ind, masks, mode))), as views of the shared per-group buffers.  whole=False leaves out the mark that lets
    decompress_tiled_batch read those buffers in place: for buffers that are only valid until their owner's next call (TiledCall)"""
    out = []
    for n in range(N):
        mine = []
        for idxs, comp, (ind, masks, mode) in groups:
            T = len(idxs)
            sl = slice(n * T, (n + 1) * T)
            per = ind.numel() // (N * T)
            mine.append((idxs, type(comp)(comp.data[sl], comp.nbytes[sl], comp.mode, comp.h, comp.w),
                         (ind.view(N * T, per)[sl].reshape(-1), [m[sl] for m in masks], mode)))
        t = TiledImage(hw, pad, tiles, mine)
        if whole:
            t._whole = (groups, n, N)             # decompress_tiled_batch of the whole list reads the shared buffers in place
        out.append(t)
    return out


def cut_groups(x, tile=TILE):
    """pad and cut N images of one size [N,3,H,W] fp32 as the tiling driver does -> (pad, tiles, order, batches): the centred pad,
    the row-major tile grid in padded coordinates, the shape groups [((th, tw), tile indices)] largest first, and per group the
    tile batch [N * T, 3, th, tw], image-major (the layout compress_tiled_batch compresses)"""
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError(f"cut_groups takes fp32 [N,3,H,W], got {x.dtype} {tuple(x.shape)}")
    N, H, W = x.shape[0], x.shape[2], x.shape[3]
    pad, tiles, order = tile_geometry(H, W, tile)
    left, _, top, _ = pad
    if len(tiles) <= 96:
        cut = _cut_all(x.contiguous(), False, N, H, W, top, left, tiles, order)
    else:
        xp = torch.nn.functional.pad(x, pad)
        cut = [torch.stack([xp[:, :, tiles[i][0]:tiles[i][0] + th, tiles[i][1]:tiles[i][1] + tw] for i in idxs], dim=1)
               for (th, tw), idxs in order]
    return pad, tiles, order, [b.reshape(-1, 3, th, tw) for b, ((th, tw), _) in zip(cut, order)]


class TiledCall:
    """The tiled driver (inference_high_resolution.py:236-257: one compress() per tile) for images of ONE size as ONE foreign call
    per image batch (cgic_compress_tiled): pad + crop + both entropy maps, VQ + per-tile router, stream coder and -- decode=True --
    decoder + merge, every link one launch for all shape groups, over buffers allocated once.  Hot path only: the latent of every
    shape group is the caller's (`zs`).  The results live in this object's buffers: valid until the next call.
    -> __call__(x, zs): x [N,3,H,W] fp32 or uint8 frames [N,H,W,3]; zs: per shape group (self.groups order: (th, tw), tile indices) the
    latent [N*T,4,th/4,tw/4]; returns a TiledImage (N == 1) or a list of N, .decoded = per group (ind, masks, z_q, status)."""

    def __init__(self, quantizer, coarse_ratio, medium_ratio, N, H, W, frequency=None, decode=True, frames=False, decoder=None, tile=TILE,
                 prepare=True):
        from .codec import GrainCodec, _decoder_flag
        from .quantize import prepare_codebook
        w = quantizer.embedding.weight
        dev = w.device
        _lib.require_device(w)
        self.vq, self.dev, self.N, self.H, self.W, self.frames = quantizer, dev, N, H, W, bool(frames)
        self.ratios = (float(coarse_ratio), float(medium_ratio))
        self.codec = GrainCodec(frequency if frequency is not None else quantizer.embedding_counter, w)
        self.prepared = prepare_codebook(w) if prepare else None
        self._prepared_version = w._version
        self.decoder = _decoder_flag(decoder)
        self.pad, self.tiles, self.groups = tile_geometry(H, W, tile)
        left, _, top, _ = self.pad
        l = _lib.lib()
        if len(self.groups) > l.cgic_group_max():
            raise ValueError(f"{len(self.groups)} tile shapes; cgic_compress_tiled takes at most {l.cgic_group_max()}")
        E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        total = sum(len(ix) * th * tw for (th, tw), ix in self.groups)
        self._arr = (_lib.TileGroup * len(self.groups))()
        self._buf, self._keep = [], []
        for k, ((th, tw), idxs) in enumerate(self.groups):
            T, B, h, ww = len(idxs), N * len(idxs), th // 4, tw // 4
            slot = self.codec.slot_bytes(h, ww)
            if not l.cgic_router_refine_in_lds(B, th // 16, tw // 16, 1):
                raise ValueError(f"TiledCall: tiles of {th}x{tw} are routed as one segment beyond the router workgroup's LDS; their refinement is a chain "
                                 "of launches that a launch group cannot record (cgic_router_refine_in_lds): use tiles of at most 768x768 "
                                 "(the reference's), or compress_tiled(..., chain=False)")
            nref = l.cgic_router_refine_scratch_bytes(B, th // 16, tw // 16, 1) if ((th // 16) * (tw // 16) >= _lib.REFINE_SPLIT_MIN_PATCHES or _lib.REFINE_FUSED_QUEUES) and _lib.REFINE_QUEUES else 0
            ws_r = E((nref,), torch.uint8) if nref else None         # (large tiles: their row bands split a threshold band between them)
            # the tile batch is the entropy pass's x_out; z_q, the loss and the histogram are not this call's
            t, io = image_io_buffers(slot, B, th, tw, decode, True, False, False, None, E, ws_refine=ws_r)
            t.update(slot=slot, h=h, w=ww)
            org = (ctypes.c_int * (2 * T))(*[v for i in idxs for v in (self.tiles[i][0] - top, self.tiles[i][1] - left)])
            g = self._arr[k]
            g.ntiles, g.th, g.tw, g.origins, g.share, g.io = T, th, tw, org, len(idxs) * th * tw / total, io
            self._buf.append(t)
            self._keep.append(org)
        self._mode = ctypes.c_int(0)
        self._fn = l.cgic_compress_tiled
        self._bins = _lib.linspace_bins()
        self._decode = bool(decode)
        self.decoded = None
        for (th, tw), _ in self.groups:               # the blend factors of paste(): uploaded here, outside any capture
            tile_weight_factors(tw, 0, dev), tile_weight_factors(th, 1, dev)

    def paste(self, pixels, out=None, frames=False):
        """the way out for this call's geometry: pixels = per shape group (self.groups order) the decoded tiles fp32 [N*T,3,th,tw]
        -> [N,3,H,W] fp32, or uint8 frames [N,H,W,3] (paste_tiles: one launch, the reference's blend + clamp + unpad).  Capturable:
        the weight factors were uploaded when this object was built; with `out` nothing is allocated"""
        left, _, top, _ = self.pad
        return _paste(pixels, self.H, self.W, top, left, self.tiles, self.groups, self.N, True, frames, out)

    def partition(self, x, out=None, frames=False):
        """the partition map of the images this call compressed last (partition_tiles for this call's geometry and its own mask
        buffers, read in place): x = the unpadded images as __call__ takes them, fp32 [N,3,H,W] or uint8 frames [N,H,W,3]
        -> fp32 [N,3,H,W], or uint8 frames [N,H,W,3].  One launch; capturable: with `out` nothing is allocated"""
        from . import draw
        _lib.require_device(x)
        _, N, H, W = draw._image_shape(x, "TiledCall.partition")
        if (N, H, W) != (self.N, self.H, self.W) or not x.is_contiguous() or x.device != self.dev:
            raise ValueError("TiledCall.partition: x does not have the shape, device or layout this object was built for")
        left, _, top, _ = self.pad
        return _partition(x, H, W, top, left, self.tiles, self.groups, [t["mask"] for t in self._buf], N, bool(frames), out)

    def refresh_codebook(self):
        """after changing embedding.weight: rewrite the codebook image in place (HotCall / HotPathPipeline have the same method; __call__
        does it by itself when the weight tensor's version counter moved)"""
        from .quantize import prepare_codebook
        if self.prepared is not None:
            self.prepared = prepare_codebook(self.vq.embedding.weight, out=self.prepared)
            self._prepared_version = self.vq.embedding.weight._version

    def __call__(self, x, zs):
        from .codec import CompressedBatch
        N, H, W = self.N, self.H, self.W
        if tuple(x.shape) != ((N, H, W, 3) if self.frames else (N, 3, H, W)) or x.dtype != (torch.uint8 if self.frames else torch.float32) \
                or not x.is_contiguous() or x.device != self.dev or len(zs) != len(self.groups):
            raise ValueError("TiledCall: x / zs do not have the shape, dtype, device or layout this object was built for")
        for k, (((th, tw), idxs), z) in enumerate(zip(self.groups, zs)):
            if tuple(z.shape) != (N * len(idxs), 4, th // 4, tw // 4) or z.dtype != torch.float32 or not z.is_contiguous() or z.device != self.dev:
                raise ValueError(f"TiledCall: latent of shape group {k} must be fp32 [{N * len(idxs)},4,{th // 4},{tw // 4}]")
            self._arr[k].io.z = z.data_ptr()
        w = self.vq.embedding.weight
        if self.prepared is not None and w._version != self._prepared_version:
            self.refresh_codebook()                 # the weights were modified in place since the image was made: a stale image gives wrong indices

        def go():
            _lib.check(self._fn(self.codec.huffman.table.handle, w.data_ptr(), w.shape[0], w.shape[1], _lib.ptr(self.prepared), x.data_ptr(),
                                int(self.frames), N, H, W, len(self.groups), self._arr, self.ratios[0], self.ratios[1], float(self.vq.beta),
                                int(bool(self.vq.legacy)), self._bins, 32, 0.01, self.decoder, ctypes.byref(self._mode),
                                torch.cuda.current_stream(self.dev).cuda_stream))
        if torch.cuda.current_device() == self.dev.index:
            go()
        else:
            with torch.cuda.device(self.dev):
                go()
        mode = self._mode.value
        groups = [(idxs, CompressedBatch(t["data"], t["nbytes"], mode, t["h"], t["w"]), (t["ind"], t["mask"], mode))
                  for (_, idxs), t in zip(self.groups, self._buf)]
        self.decoded = [(t["dind"], t["dmask"], t["dz_q"], t["status"]) for t in self._buf] if self._decode else None
        if N == 1:
            return TiledImage((H, W), self.pad, self.tiles, groups)
        return assemble_tiled((H, W), self.pad, self.tiles, groups, N, whole=False)


def _decompress_chain(comps, codec, dev, decoder):
    """chain=True of the two decompress drivers: the decoder and the merge of all shape groups (`comps`: one CompressedBatch each) as ONE
    launch each (see compress_tiled), and one status buffer for all of them: no concatenation kernel afterwards
    -> ([(ind, masks, z_q, status) per group], the status of all groups)"""
    status_all = torch.empty(sum(c.batch for c in comps), dtype=torch.int32, device=dev)
    outs, at = [], 0
    with _lib.launch_group(len(comps), [c.batch * c.h * c.w for c in comps], dev) as g:
        for k, comp in enumerate(comps):
            g.select(k)
            outs.append(codec.decompress(comp, status=status_all[at:at + comp.batch], decoder=decoder))
            at += comp.batch
    return outs, status_all


def decompress_tiled_batch(tiled_list, codec, concurrent=False, check=True, chain=False, decoder=None, decode=None, frames=False):
    """inverse of compress_tiled_batch for TiledImages of one geometry (from it, or from N compress_tiled calls on images
    of one size, or rebuilt from containers by container.load(...).tiled(hw)): ONE decompress per shape group over all the images
    -> list (per image) of per-tile (ind, masks, z_q); check=False: (that, [N * tiles] status tensor).
    decode(z_q [N*T,4,h,w], masks) -> pixels [N*T,3,th,tw]: called ONCE per shape group on the whole batch (not once per tile), then all
    tiles of all images are pasted in one launch (paste_tiles: the reference's blend + clamp + unpad, :248-255) -> (per_image, rec) with
    rec [N,3,H,W] fp32, or with frames=True the uint8 frames [N,H,W,3] write_images would save; check=False: (per_image, rec, status)"""
    if not tiled_list:
        return [] if decode is None else ([], None)
    first = tiled_list[0]
    for t in tiled_list[1:]:
        if t.tiles != first.tiles or [g[0] for g in t.groups] != [g[0] for g in first.groups] or \
                any(a[1].mode != b[1].mode for a, b in zip(t.groups, first.groups)):
            raise ValueError("decompress_tiled_batch: the images differ in geometry or routing mode")
    N = len(tiled_list)
    per_image = [[None] * len(first.tiles) for _ in range(N)]
    dev = first.groups[0][1].data.device
    chain = chain and 1 < len(first.groups) <= _lib.lib().cgic_group_max()
    fork = _Fork(dev, concurrent and not chain)
    outs, statuses = [], []
    pending = []
    whole = getattr(first, "_whole", None)
    if whole is not None and not (whole[2] == N and all(
            getattr(t, "_whole", (None,))[0] is whole[0] and t._whole[1] == n for n, t in enumerate(tiled_list))):
        whole = None
    for lane, (idxs, c0, _) in enumerate(first.groups):
        with fork.on(lane):
            if whole is not None:
                comp = whole[0][lane][1]
            else:
                comps = [t.groups[lane][1] for t in tiled_list]
                slot = max(c.data.shape[-1] for c in comps)
                data = torch.cat([c.data if c.data.shape[-1] == slot else
                                  torch.nn.functional.pad(c.data, (0, slot - c.data.shape[-1])) for c in comps])
                comp = type(c0)(data, torch.cat([c.nbytes for c in comps]), c0.mode, c0.h, c0.w)
            if chain:
                pending.append(comp)
                continue
            outs.append(codec.decompress(comp, decoder=decoder))
    status_all = None
    if chain:
        outs, status_all = _decompress_chain(pending, codec, dev, decoder)
    for (idxs, _, _), (ind, masks, zq, status) in zip(first.groups, outs):
        statuses.append(status)
        T = len(idxs)
        for n in range(N):
            for k, i in enumerate(idxs):
                j = n * T + k
                per_image[n][i] = (ind[j:j + 1], [m[j:j + 1] for m in masks], zq[j:j + 1])
    fork.join(outs)
    all_status = status_all if status_all is not None else torch.cat(statuses)
    if check and int(all_status.abs().max()) != 0:
        raise RuntimeError("corrupt tile stream")
    if decode is None:
        return per_image if check else (per_image, all_status)
    pixels = [decode(zq, masks).contiguous() for _, masks, zq, _ in outs]          # ONE decoder call per shape group
    left, _, top, _ = first.pad
    rec = _paste(pixels, first.image_hw[0], first.image_hw[1], top, left, first.tiles, first.shape_groups(), N, True, frames, None)
    return (per_image, rec) if check else (per_image, rec, all_status)


def decompress_tiled(tiled, codec, decode=None, concurrent=False, check=True, chain=False, decoder=None):
    """-> per-tile (ind, masks, z_q) in row-major order; with decode(z_q, masks) -> pixels also the blended,
    clamped, unpadded reconstruction (:248-255; tiles do not overlap, so the weights cancel).
    concurrent: shape groups on parallel streams; check=False skips the host synchronisation on the decoder status (for
    stream capture): the second result is then the [tiles] status tensor to look at later.
    decoder: "latency" / "throughput" / "auto" (GrainCodec.decompress).  "latency" = this call has the GPU to itself: with chain the
    decoder and the merge of ALL shape groups are then one launch; the default keeps that form to launches of at most half the
    chip (several decode chains in flight on other streams must never leave a merge band spinning on a decoder without a CU)."""
    per_tile = [None] * len(tiled.tiles)
    statuses = []
    dev = tiled.groups[0][1].data.device if tiled.groups else None
    chain = chain and dev is not None and 1 < len(tiled.groups) <= _lib.lib().cgic_group_max()
    fork = _Fork(dev, concurrent and dev is not None and not chain)
    outs, status_all = _decompress_chain([c for _, c, _ in tiled.groups], codec, dev, decoder) if chain else ([], None)
    for lane, (idxs, comp, _) in enumerate(tiled.groups):
        if not chain:
            with fork.on(lane):
                outs.append(codec.decompress(comp, decoder=decoder))
        ind, masks, zq, status = outs[lane]
        statuses.append(status)
        for k, i in enumerate(idxs):
            per_tile[i] = (ind[k:k + 1], [m[k:k + 1] for m in masks], zq[k:k + 1])
    fork.join(outs)
    all_status = status_all if status_all is not None else (torch.cat(statuses) if statuses else None)
    if not check:
        return per_tile, all_status
    # ONE host synchronisation for the whole image (not one per shape group)
    if all_status is not None and int(all_status.abs().max()) != 0:
        raise RuntimeError("corrupt tile stream")
    if decode is None:
        return per_tile, None
    H, W = tiled.image_hw
    left, right, top, bottom = tiled.pad
    dev = per_tile[0][2].device
    rec = torch.zeros((1, 3, H + top + bottom, W + left + right), device=dev)
    contrib = torch.zeros_like(rec)
    for (y, x, th, tw), (ind, masks, zq) in zip(tiled.tiles, per_tile):
        wts = gaussian_weights(tw, th, dev)
        rec[:, :, y:y + th, x:x + tw] += decode(zq, masks) * wts                 # :248 (float32 += float64 product)
        contrib[:, :, y:y + th, x:x + tw] += wts
    rec = (rec / contrib).clamp(0, 1)
    return per_tile, rec[:, :, top:top + H, left:left + W]
