"""A container format for batches and tiled images.

The reference writes five fixed-name files per compress() call and overwrites them for every image and
every tile (model.py:226-249, inference_high_resolution.py:246), so nothing but the last tile of the last
image survives on disk.  This container keeps every entry decodable:

    magic  "CGIC"  | u16 version = 1 | u16 flags = 0 | u32 n_entries
    n_entries x entry header (44 bytes, little endian):
        u32 image_id | u32 y | u32 x | u32 height | u32 width   (pixel rectangle in the padded image)
        u8 mode | 3 pad bytes | 5 x i32 stream length (-1 = stream not written in this mode)
    payload: the streams of entry 0 (in stream order), entry 1, ...  byte-identical to the reference's .bin files

`write_legacy` in codec.py still produces the reference's own five files for one image.
"""
import struct

from ._lib import STREAM_NAMES

MAGIC = b"CGIC"
VERSION = 1
_HDR = struct.Struct("<4sHHI")
_ENT = struct.Struct("<IIIIIB3x5i")


def pack(entries):
    """entries: list of dict(image_id, y, x, height, width, mode, streams={name: bytes}) -> bytes"""
    head = [_HDR.pack(MAGIC, VERSION, 0, len(entries))]
    body = []
    for e in entries:
        lens = [len(e["streams"][n]) if n in e["streams"] else -1 for n in STREAM_NAMES]
        head.append(_ENT.pack(e["image_id"], e["y"], e["x"], e["height"], e["width"], e["mode"], *lens))
        body.extend(e["streams"][n] for n in STREAM_NAMES if n in e["streams"])
    return b"".join(head + body)


def unpack(blob):
    magic, version, _flags, n = _HDR.unpack_from(blob, 0)
    if magic != MAGIC or version != VERSION:
        raise ValueError("not a CGIC container (or unknown version)")
    off = _HDR.size
    metas = []
    for _ in range(n):
        metas.append(_ENT.unpack_from(blob, off))
        off += _ENT.size
    out = []
    for image_id, y, x, hh, ww, mode, *lens in metas:
        streams = {}
        for name, ln in zip(STREAM_NAMES, lens):
            if ln >= 0:
                if off + ln > len(blob):
                    raise ValueError("truncated container")
                streams[name] = bytes(blob[off:off + ln])
                off += ln
        out.append(dict(image_id=image_id, y=y, x=x, height=hh, width=ww, mode=mode, streams=streams))
    if off != len(blob):
        raise ValueError("trailing bytes after the last stream")
    return out


def entries_from_batch(comp, height, width, first_image_id=0):
    """CompressedBatch of whole images -> container entries"""
    return [dict(image_id=first_image_id + b, y=0, x=0, height=height, width=width, mode=comp.mode, streams=s)
            for b, s in enumerate(comp.to_host())]


def entries_from_tiled(tiled, image_id=0):
    """TiledImage -> container entries, row-major tile order"""
    modes = [None] * len(tiled.tiles)
    for idxs, comp, _ in tiled.groups:
        for i in idxs:
            modes[i] = comp.mode
    return [dict(image_id=image_id, y=y, x=x, height=th, width=tw, mode=modes[i], streams=s)
            for i, ((y, x, th, tw), s) in enumerate(zip(tiled.tiles, tiled.streams()))]


def bits_per_pixel(entries, image_hw):
    """sum of stream bytes * 8 / (H * W) -- equals the reference's bpp accounting for whole images and tiles"""
    return sum(len(v) for e in entries for v in e["streams"].values()) * 8 / (image_hw[0] * image_hw[1])


# ---- the device side (csrc/cgic_container.hip, ABI 15): the same blob without a host loop -------------------------------------
# pack_device builds the blob from slot buffers on the device (no synchronisation: it can follow a compress inside a captured graph);
# load uploads a file once and scatters it into slot buffers the decoders accept.  pack / unpack above stay the CPU reference.

def parse_header(blob):
    """the header of a container without touching its payload, vectorised -> dict of numpy arrays: image_id, y, x, height, width,
    mode ([E]), lens ([E,5] int32, -1 = stream not written), offsets ([E,5] int64: where each stream starts in the blob -- for a
    stream not written: where it would), and the ints n_entries, payload_start, size.  ValueError where `unpack` refuses the blob
    (magic, version, truncated, trailing bytes) and for a length below -1 or lengths that do not add up to the blob's size"""
    import numpy as np
    buf = np.frombuffer(blob, dtype=np.uint8)
    if buf.size < _HDR.size:
        raise ValueError("truncated container (no header)")
    magic, version, _flags, n = _HDR.unpack_from(blob, 0)
    if magic != MAGIC or version != VERSION:
        raise ValueError("not a CGIC container (or unknown version)")
    start = _HDR.size + _ENT.size * n
    if buf.size < start:
        raise ValueError("truncated container (entry headers)")
    ent = np.dtype([("image_id", "<u4"), ("y", "<u4"), ("x", "<u4"), ("height", "<u4"), ("width", "<u4"), ("mode", "u1"), ("pad", "u1", 3),
                    ("lens", "<i4", 5)])
    assert ent.itemsize == _ENT.size
    tab = np.frombuffer(blob, dtype=ent, count=n, offset=_HDR.size)
    lens = tab["lens"].astype(np.int32).reshape(n, 5)
    if n and int(lens.min()) < -1:
        raise ValueError("a stream length below -1")
    sizes = np.maximum(lens, 0).astype(np.int64).reshape(-1)
    ends = np.cumsum(sizes) + start
    total = int(ends[-1]) if n else start
    if total > buf.size:
        raise ValueError("truncated container")
    if total < buf.size:
        raise ValueError("trailing bytes after the last stream")
    out = {k: tab[k].astype(np.int64) for k in ("image_id", "y", "x", "height", "width", "mode")}
    out.update(lens=lens, offsets=(ends - sizes).reshape(n, 5), n_entries=int(n), payload_start=start, size=int(buf.size))
    return out


def _raise_negative(v, what):
    """a negative `total` of cgic_container_pack, raised as CompressedBatch.to_host() raises the nbytes word behind it"""
    from . import _lib
    bad = int(v) + 10
    if bad == _lib.ERR_INVALID:
        raise KeyError("a symbol is not in the code table")
    if bad == _lib.ERR_CAPACITY:
        raise _lib.CgicError(bad, f"{what}: the container does not fit the blob's capacity (or a stream is longer than its slot)")
    raise _lib.CgicError(bad, f"{what}: compress_streams failed on the device")


class PackedContainer:
    """result of pack_device: blob uint8 [capacity] and total int64 [1] on the device (total < 0: see cgic_container_pack).  Nothing
    has synchronised yet; a replay of a captured pack_device rewrites both"""

    def __init__(self, blob, total):
        self.blob, self.total = blob, total

    def nbytes(self):
        """the size of the container (synchronises); raises as CompressedBatch.to_host() does when the compress behind it failed"""
        n = int(self.total.cpu()[0])
        if n < 0:
            _raise_negative(n, "pack_device")
        return n

    def tobytes(self):
        """the container as bytes == container.pack of the same entries: reads `total`, then ONE contiguous copy of blob[:total]"""
        return self.blob[:self.nbytes()].cpu().numpy().tobytes()


def _table_args(groups, entries):
    import ctypes
    from . import _lib
    G, E = len(groups), len(entries)
    # (the limits are the library's to refuse; the ctypes arrays only have to exist)
    garr = (_lib.ContainerGroup * max(G, 1))()
    for k, c in enumerate(groups):
        if c.data.dtype.itemsize != 1 or c.data.dim() != 3 or c.data.shape[1] != _lib.NUM_STREAMS or not c.data.is_contiguous() \
                or tuple(c.nbytes.shape) != (c.data.shape[0], _lib.NUM_STREAMS) or c.nbytes.dtype.itemsize != 4 or not c.nbytes.is_contiguous():
            raise ValueError(f"container: group {k} must be contiguous data uint8 [B,5,slot] with nbytes int32 [B,5]")
        garr[k] = _lib.ContainerGroup(c.data.data_ptr(), c.nbytes.data_ptr(), c.data.shape[0], c.data.shape[2], int(c.mode))
    earr = (_lib.ContainerEntry * max(E, 1))()
    lim = 1 << 32
    for k, e in enumerate(entries):
        if not all(0 <= int(v) < lim for v in e[:5]) or not all(-(1 << 31) <= int(v) < (1 << 31) for v in e[5:]):
            raise ValueError(f"container: entry {k} does not fit the header's 32-bit fields")
        earr[k] = _lib.ContainerEntry(*[int(v) for v in e])
    return garr, G, earr, E, ctypes


def pack_groups(groups, entries, blob=None, total=None):
    """cgic_container_pack on explicit tables: groups = CompressedBatches (their data / nbytes are read in place), entries = tuples
    (image_id, y, x, height, width, group, index in group) in container order -> PackedContainer.  blob (uint8, its length is the
    capacity) and total (int64 [1]) may be given; by default the blob gets 12 + 44 E + five slots of its own group per entry, which
    always suffices.  Every argument is checked before anything is enqueued; nothing synchronises"""
    import torch
    from . import _lib
    garr, G, earr, E, _ = _table_args(groups, entries)
    dev = groups[0].data.device if groups else (blob.device if blob is not None else torch.device("cuda", torch.cuda.current_device()))
    _lib.require_device(*[t for c in groups for t in (c.data, c.nbytes)], blob, total)
    if blob is None:
        cap = _HDR.size + _ENT.size * E + sum(_lib.NUM_STREAMS * groups[e[5]].data.shape[2] for e in entries if 0 <= e[5] < G)
        blob = torch.empty(cap, dtype=torch.uint8, device=dev)
    elif blob.dtype != torch.uint8 or blob.dim() != 1 or not blob.is_contiguous() or blob.device != dev:
        raise ValueError("pack_device: blob must be a contiguous 1-D uint8 tensor on the streams' device")
    if total is None:
        total = torch.empty(1, dtype=torch.int64, device=dev)
    elif total.dtype != torch.int64 or total.numel() != 1 or total.device != dev:
        raise ValueError("pack_device: total must be int64 [1] on the streams' device")
    ws = torch.empty(max(int(_lib.lib().cgic_container_workspace_bytes(min(E, 65535))), 16), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.call("cgic_container_pack", garr, G, earr, E, _lib.ptr(blob), blob.numel(), _lib.ptr(total), _lib.ptr(ws), _lib.current_stream(dev))
    return PackedContainer(blob, total)


def _tables_of(items, height, width, first_image_id):
    """the group and entry tables of pack_device's items"""
    from .highres import TiledImage
    groups, entries, seen = [], [], {}

    def group_of(comp):
        key = (comp.data.data_ptr(), comp.nbytes.data_ptr(), comp.data.shape[0])
        if key not in seen:
            seen[key] = len(groups)
            groups.append(comp)
        return seen[key]

    def tiled(t, image_id, whole):
        where = [None] * len(t.tiles)
        for lane, (idxs, comp, _) in enumerate(t.groups):
            if whole is not None:                       # the shared buffer of the shape group, image-major: read in place
                shared, n = whole[0][lane][1], whole[1]
                g, at = group_of(shared), n * len(idxs)
            else:
                g, at = group_of(comp), 0
            for k, i in enumerate(idxs):
                where[i] = (g, at + k)
        for (y, x, th, tw), (g, index) in zip(t.tiles, where):
            entries.append((image_id, y, x, th, tw, g, index))

    if not isinstance(items, (list, tuple)):
        items = [items]
    elif len(items) > 1 and all(isinstance(t, TiledImage) and getattr(t, "_whole", None) is not None for t in items):
        items = [items]                                 # the list of compress_tiled_batch itself: as one nested list
    image_id = int(first_image_id)
    for it in items:
        if isinstance(it, (list, tuple)):               # the list compress_tiled_batch returns (or any list of TiledImages)
            w0 = getattr(it[0], "_whole", None) if it else None
            shared = w0 is not None and w0[2] == len(it) and all(
                getattr(t, "_whole", (None,))[0] is w0[0] and t._whole[1] == n for n, t in enumerate(it))
            for t in it:
                if not isinstance(t, TiledImage):
                    raise TypeError("pack_device: a nested list holds TiledImages")
                tiled(t, image_id, t._whole if shared else None)
                image_id += 1
        elif isinstance(it, TiledImage):
            tiled(it, image_id, None)
            image_id += 1
        else:                                           # a CompressedBatch of whole images
            g = group_of(it)
            hh, ww = (4 * it.h if height is None else int(height)), (4 * it.w if width is None else int(width))
            for b in range(it.batch):
                entries.append((image_id, 0, 0, hh, ww, g, b))
                image_id += 1
    return groups, entries


def pack_device(items, height=None, width=None, first_image_id=0, blob=None, total=None):
    """the container of `items`, built on the device (cgic_container_pack) -> PackedContainer; .tobytes() == pack(entries) of the
    same items, byte for byte.  items: a CompressedBatch of whole images (entries as entries_from_batch(comp, height, width,
    first_image_id); height / width default to 4 x the latent grid), a TiledImage (entries as entries_from_tiled), a list of
    TiledImages as compress_tiled_batch returns it (the shared per-group buffers are read in place), or a list of any of these:
    image ids count up from first_image_id -- one per image of a batch, one per tiled image.
    Nothing is copied to the host and nothing synchronises before .tobytes() / .nbytes(): the call can follow a compress inside a
    captured graph and be replayed (its group and entry tables are part of the recorded launches)"""
    groups, entries = _tables_of(items, height, width, first_image_id)
    return pack_groups(groups, entries, blob=blob, total=total)


class LoadedContainer:
    """result of load: .entries = parse_header's dict; .groups = [(entry indices, CompressedBatch)], entries grouped by
    (height, width, mode) in order of first appearance, each group's images in container order"""

    def __init__(self, entries, groups):
        self.entries, self.groups = entries, groups

    def batch(self):
        """the one CompressedBatch of a container of whole images of one shape and mode (GrainCodec.decompress takes it)"""
        e = self.entries
        if len(self.groups) != 1 or int(e["y"].max()) != 0 or int(e["x"].max()) != 0:
            raise ValueError("LoadedContainer.batch: the entries are not whole images of one shape and mode")
        return self.groups[0][1]

    def tiled(self, image_hw, tile=None):
        """-> list of TiledImage, one per image_id in order of first appearance, for decompress_tiled / decompress_tiled_batch.
        image_hw = (H, W) of the UNPADDED image (the format does not hold it); the pad is compute_padding(H, W), and the rectangles
        of every image must be exactly tile_grid of the padded size (ValueError otherwise).  tile: the grid's tile size; None = what
        the entry at (0, 0) says (its width if there are several columns, else its height if there are several rows).  Where all
        the images share one geometry the TiledImages are views of the groups' buffers, image-major, and decompress_tiled_batch
        reads them in place"""
        import torch
        from . import highres
        from .codec import CompressedBatch
        e = self.entries
        H, W = int(image_hw[0]), int(image_hw[1])
        pad, _ = highres.compute_padding(H, W)
        left, right, top, bottom = pad
        ph, pw = H + top + bottom, W + left + right
        ids = []
        by_image = {}
        for k, v in enumerate(e["image_id"].tolist()):
            if v not in by_image:
                by_image[v] = []
                ids.append(v)
            by_image[v].append(k)
        where = {}                                       # entry -> (group, index in group)
        for g, (idxs, _) in enumerate(self.groups):
            for j, k in enumerate(idxs):
                where[k] = (g, j)
        rect = lambda k: (int(e["y"][k]), int(e["x"][k]), int(e["height"][k]), int(e["width"][k]))
        per_image = []
        for v in ids:
            mine = {rect(k): k for k in by_image[v]}
            t = tile
            if t is None:
                first = mine.get(next((r for r in mine if r[0] == 0 and r[1] == 0), None))
                if first is None:
                    raise ValueError(f"LoadedContainer.tiled: image {v} has no tile at (0, 0)")
                t = rect(first)[3] if any(r[1] > 0 for r in mine) else rect(first)[2] if any(r[0] > 0 for r in mine) else max(highres.TILE, ph, pw)
            _, tiles, order = highres.tile_geometry(H, W, int(t))
            if len(mine) != len(by_image[v]) or sorted(mine) != sorted(tiles):
                raise ValueError(f"LoadedContainer.tiled: the rectangles of image {v} are not the tile grid of a {H}x{W} image "
                                 f"(padded {ph}x{pw}, tile {t})")
            lanes = []
            for (th, tw), idxs in order:
                at = [where[mine[tiles[i]]] for i in idxs]
                if len({g for g, _ in at}) != 1:
                    raise ValueError(f"LoadedContainer.tiled: the {th}x{tw} tiles of image {v} were written in different modes")
                lanes.append((idxs, at[0][0], [j for _, j in at]))
            per_image.append((tiles, lanes))
        N = len(per_image)
        # in place: every image the same grid, and lane by lane its tiles at [n T, (n + 1) T) of ONE group that holds nothing else
        shared = N > 0 and all(p[0] == per_image[0][0] and [(l[0], l[1]) for l in p[1]] == [(l[0], l[1]) for l in per_image[0][1]]
                               for p in per_image) and all(
            self.groups[lane[1]][1].batch == N * len(lane[0]) and lane[2] == list(range(n * len(lane[0]), (n + 1) * len(lane[0])))
            for n, p in enumerate(per_image) for lane in p[1])
        whole = [(idxs, self.groups[g][1], None) for idxs, g, _ in per_image[0][1]] if shared else None
        out = []
        for n, (tiles, lanes) in enumerate(per_image):
            groups = []
            for idxs, g, js in lanes:
                c = self.groups[g][1]
                if shared:
                    sl = slice(js[0], js[-1] + 1)
                    groups.append((idxs, CompressedBatch(c.data[sl], c.nbytes[sl], c.mode, c.h, c.w), None))
                else:
                    sel = torch.tensor(js, dtype=torch.int64, device=c.data.device)
                    groups.append((idxs, CompressedBatch(c.data.index_select(0, sel), c.nbytes.index_select(0, sel), c.mode, c.h, c.w), None))
            t = highres.TiledImage((H, W), pad, tiles, groups)
            if shared:
                t._whole = (whole, n, N)
            out.append(t)
        return out


def load(blob, codec, device, fill=None):
    """a container (bytes) -> LoadedContainer whose CompressedBatches GrainCodec.decompress / decompress_tiled_batch accept: ONE
    upload of the file and one cgic_container_unpack.  Entries are grouped by (height, width, mode) in order of first appearance;
    a group's slot is codec.slot_bytes of its latent grid (height / 4, width / 4).  ValueError before anything is uploaded: what
    parse_header refuses, a rectangle whose sides are no multiples of 16, a mode outside 0 .. 6, streams that are not the set the
    entry's mode writes, a stream that does not fit its slot.
    fill: None leaves the bytes of a slot behind a stream's zeroed slack as allocated; a byte value presets the slots (tests)"""
    import torch
    from . import _lib
    from .codec import CompressedBatch, mode_streams
    meta = parse_header(blob)
    E = meta["n_entries"]
    if E > 65535:
        raise ValueError("load: more than 65535 entries")
    keys, members = {}, []
    entries = []
    for k in range(E):
        hh, ww, mode = int(meta["height"][k]), int(meta["width"][k]), int(meta["mode"][k])
        if hh <= 0 or ww <= 0 or hh % 16 or ww % 16:
            raise ValueError(f"load: entry {k} is {hh}x{ww} pixels: the sides of an image or tile are multiples of 16")
        if not 0 <= mode <= 6:
            raise ValueError(f"load: entry {k} has routing mode {mode}")
        g = keys.setdefault((hh, ww, mode), len(keys))
        if g == len(members):
            members.append([])
        entries.append((0, 0, 0, 0, 0, g, len(members[g])))
        members[g].append(k)
    if len(keys) > 64:
        raise ValueError(f"load: {len(keys)} different (height, width, mode); one call takes 64")
    slots = []
    for (hh, ww, mode), g in keys.items():
        on = mode_streams(mode)
        lens = meta["lens"][members[g]]
        if ((lens >= 0) != [bool(v) for v in on]).any():
            raise ValueError(f"load: an entry of mode {mode} does not hold the streams that mode writes")
        slot = codec.slot_bytes(hh // 4, ww // 4)
        if int(lens.max()) + 8 > slot:
            raise ValueError(f"load: a stream of {int(lens.max())} B does not fit the slot of a {hh}x{ww} entry ({slot} B)")
        slots.append(slot)
    dev = torch.device(device)
    _lib.require_device(torch.empty(0, device=dev))
    host = torch.frombuffer(bytearray(blob), dtype=torch.uint8)
    dblob = torch.empty((host.numel() + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    dblob[:host.numel()].copy_(host)                                    # the one upload
    groups = []
    for ((hh, ww, mode), g), slot in zip(keys.items(), slots):
        shape = (len(members[g]), _lib.NUM_STREAMS, slot)
        data = torch.empty(shape, dtype=torch.uint8, device=dev) if fill is None else torch.full(shape, int(fill), dtype=torch.uint8, device=dev)
        nbytes = torch.empty((len(members[g]), _lib.NUM_STREAMS), dtype=torch.int32, device=dev)
        groups.append((members[g], CompressedBatch(data, nbytes, mode, hh // 4, ww // 4)))
    if E:
        garr, G, earr, _, ctypes = _table_args([c for _, c in groups], entries)
        ws = torch.empty(int(_lib.lib().cgic_container_workspace_bytes(E)), dtype=torch.uint8, device=dev)
        hbuf = blob if isinstance(blob, bytes) else bytes(blob)            # (ctypes passes the address of a bytes object's buffer)
        with _lib.on_device(dev):
            _lib.call("cgic_container_unpack", hbuf, _lib.ptr(dblob), len(blob), garr, G, earr, E, _lib.ptr(ws), _lib.current_stream(dev))
    return LoadedContainer(meta, groups)
