"""Partition maps -- the hot-path side of CGIC/modules/draw.py: where the router spent coarse, medium and fine codes.

The reference draws the grain grid with three nested Python loops and two strided slice assignments per cell
(draw_triple_grain_256res, draw.py:78-119: 5376 cells per 256x256 image, about 220 000 for a 2040x1356 one).  Per pixel the loops are
a select between the image value and -1 (the closed form in include/cgic_hip.h); here it is ONE launch for a whole batch
(cgic_partition_map), bit-identical to the loops on the CPU.

    draw_triple_grain_256res(images, indices)    the reference's function: draws into `images` in place, any [B,gh,gw] indices
    partition_map(x, mask)                       the same picture straight from the router's three masks
    grain_map(mask)                              the [B,h,w] 0/1/2 indices of the masks (plain torch), for the reference's own drawers

Deliberate deviation: model.compress(save_img=True) draws the routing that was actually USED, from the masks.  The
stock encoder's `grain_indices` (vqvae_blocks.py:357-359) is a permute of a [B,1,h,3w] gate followed by an argmax over the wrong axis:
a [B,1,h] tensor with values up to 3w-1, whose picture is a few meaningless lines.  draw_triple_grain_256res(x.clone(), grain_indices)
on that tensor reproduces the reference's picture bit for bit for whoever needs it.

draw_triple_grain_256res_color (a PIL blend, commented out at model.py:418) is out of scope.
"""
import torch

from . import _lib

MAX_TILES = 84          # tiles of one cgic_partition_map launch (what fits its 4 KB argument block); more are split here


def grain_map(mask):
    """the router's three masks ([B,1,h/4,w/4], [B,1,h/2,w/2], [B,1,h,w], or without the singleton axis) -> int64 [B,h,w] of 0 (coarse),
    1 (medium), 2 (fine): the FIRST maximum over (up4(mask[0]), up2(mask[1]), mask[2]) with a nonzero element counting as 1 -- what
    the comment at vqvae_blocks.py:358 means and what `argmax` gives: coarse wins, then medium, then fine; all zero -> 0.  Plain
    torch operations on whatever device the masks live on; the result is what the reference's own drawers and log_images take."""
    mc, mm, mf = mask
    B, h, w = mf.shape[0], mf.shape[-2], mf.shape[-1]
    if h % 4 or w % 4 or mc.numel() != B * (h // 4) * (w // 4) or mm.numel() != B * (h // 2) * (w // 2) or mf.numel() != B * h * w:
        raise ValueError("grain_map: masks at 1/4, 1/2 and 1/1 of a fine grid whose sides are multiples of 4")
    c = (mc.reshape(B, h // 4, w // 4) != 0).repeat_interleave(4, 1).repeat_interleave(4, 2)
    m = (mm.reshape(B, h // 2, w // 2) != 0).repeat_interleave(2, 1).repeat_interleave(2, 2)
    f = mf.reshape(B, h, w) != 0
    return (~c & m).to(torch.int64) + 2 * (~c & ~m & f).to(torch.int64)


def _image_shape(x, what):
    """(frames, N, H, W) of fp32 [N,3,H,W] or uint8 frames [N,H,W,3]"""
    if x.dim() == 4 and x.dtype == torch.uint8 and x.shape[3] == 3:
        return True, x.shape[0], x.shape[1], x.shape[2]
    if x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3:
        return False, x.shape[0], x.shape[2], x.shape[3]
    raise ValueError(f"{what}: expected fp32 [N,3,H,W] or uint8 frames [N,H,W,3], got {x.dtype} {tuple(x.shape)}")


def _launch(x, N, H, W, desc, frames, out, what):
    """cgic_partition_map on contiguous `x` (fp32 [*,3,H,W] or uint8 [*,H,W,3]; the first N images) for the tile descriptors `desc`
    -> out (allocated when None: fp32 [N,3,H,W], or with frames uint8 [N,H,W,3])"""
    want, dt = ((N, H, W, 3), torch.uint8) if frames else ((N, 3, H, W), torch.float32)
    if out is None:
        out = torch.empty(want, dtype=dt, device=x.device)
    elif tuple(out.shape) != want or out.dtype != dt or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"{what}: out must be contiguous {dt} {list(want)} on {x.device}")
    with _lib.on_device(x.device):
        stream = _lib.current_stream(x.device)
        for at in range(0, len(desc), MAX_TILES):
            part = desc[at:at + MAX_TILES]
            _lib.call("cgic_partition_map", x.data_ptr(), int(x.dtype == torch.uint8), N, H, W, len(part), (_lib.PartitionTile * len(part))(*part),
                      None if frames else out.data_ptr(), out.data_ptr() if frames else None, stream)
    return out


def _check_masks(mask, B, H, W, what):
    mask = list(mask)
    if len(mask) != 3:
        raise ValueError(f"{what}: mask = the router's three tensors (coarse, medium, fine)")
    _lib.require_device(*mask)
    _lib.require_int32_masks(*mask)
    if H % 16 or W % 16:
        raise ValueError(f"{what}: the router's masks belong to images whose sides are multiples of 16, got {H}x{W}")
    for m, d in zip(mask, (16, 8, 4)):
        if m.numel() != B * (H // d) * (W // d) or m.shape[0] != B or tuple(m.shape[-2:]) != (H // d, W // d):
            raise ValueError(f"{what}: mask {tuple(m.shape)} does not belong to {B} images of {H}x{W} (expected [{B},1,{H // d},{W // d}])")
    return [m.contiguous() for m in mask]


def partition_map(x, mask, frames=False, out=None):
    """the partition map of a batch in ONE launch: x = fp32 [B,3,H,W] or uint8 frames [B,H,W,3], mask = the router's three int32
    masks of it -> fp32 [B,3,H,W] (line pixels -1, the reference's picture: draw_triple_grain_256res on grain_map(mask)), or with
    frames=True the uint8 frames [B,H,W,3] write_images would save (line pixels 1, see include/cgic_hip.h).  `x` is never modified
    unless `out is x`.  With `out` (that shape, contiguous) nothing is allocated and nothing synchronises: capturable."""
    _lib.require_device(x)
    _, B, H, W = _image_shape(x, "partition_map")
    mc, mm, mf = _check_masks(mask, B, H, W, "partition_map")
    if any(m.device != x.device for m in (mc, mm, mf)):
        raise ValueError("partition_map: the masks and the image live on different devices")
    if out is x and not x.is_contiguous():
        raise ValueError("partition_map: an in-place draw needs a contiguous image")
    xc = x.contiguous()
    desc = [_lib.PartitionTile(_lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf), None, 1, 0, 0, H, W, 0, 0)]
    return _launch(xc, B, H, W, desc, bool(frames), out, "partition_map")


def draw_triple_grain_256res(images=None, indices=None):
    """CGIC/modules/draw.py:78-119 with the reference's signature and contract: draws the grain grid of `indices` ([B,gh,gw], any
    integer dtype, any values: 1 = medium, 2 = fine, coarse lines always; the stock encoder's malformed [B,1,h] tensor included)
    into `images` (fp32 [B,3,H,W] on the device, contiguous) IN PLACE as -1 and returns it.  One launch.  Like the reference it draws
    the first indices.size(0) images; a grid finer than the image (H // gh == 0) is refused."""
    if images is None or indices is None:
        raise TypeError("draw_triple_grain_256res needs images and indices (the reference's `images=None` path fails at draw.py:81)")
    _lib.require_device(images, indices)
    frames, B, H, W = _image_shape(images, "draw_triple_grain_256res")
    if frames:
        raise ValueError("draw_triple_grain_256res takes fp32 [B,3,H,W] like the reference's; partition_map draws into uint8 frames")
    if not images.is_contiguous():
        raise ValueError("draw_triple_grain_256res draws in place: the image batch must be contiguous")
    if indices.dim() != 3 or indices.is_floating_point() or indices.dtype == torch.bool or indices.is_complex():
        raise ValueError(f"draw_triple_grain_256res: indices must be an integer tensor [B,gh,gw], got {indices.dtype} {tuple(indices.shape)}")
    if indices.shape[0] > B:
        raise IndexError(f"draw_triple_grain_256res: indices of {indices.shape[0]} images for a batch of {B}")
    if indices.device != images.device:
        raise ValueError("draw_triple_grain_256res: indices and images live on different devices")
    n, gh, gw = indices.shape
    if n == 0:
        return images
    idx = indices.to(torch.int64).contiguous()
    desc = [_lib.PartitionTile(None, None, None, _lib.ptr(idx), 1, 0, 0, H, W, gh, gw)]
    head = images if n == B else images[:n]                    # (a leading slice of a contiguous batch: contiguous, same storage)
    _launch(images, n, H, W, desc, False, head, "draw_triple_grain_256res")
    return images
