"""CPU expectations for the partition-map tests (numpy only; never the kernel under test, never GPU torch operations).

Two sources: `loop_draw`, a restatement of the three cell loops of CGIC/modules/draw.py:78-119 as per-cell slice assignments (small
shapes), and `closed_form`, the vectorised closed form of include/cgic_hip.h (large shapes).  tests/test_partition_host.py holds
the closed form to the loops and both to the fixture of the real function (tests/golden/partition.npz)."""
import numpy as np

from control_gic_amd import highres


def loop_draw(images, indices):
    """images [B,3,H,W] (any dtype) drawn on a copy: every cell paints its top row and its left column with -1 -- coarse cells
    (4x4 index cells) always, medium cells (2x2) where their top-left index is 1, fine cells where their index is 2"""
    pic = images.copy()
    H, W = pic.shape[-2:]
    n, gh, gw = indices.shape
    ch, cw = H // gh, W // gw                                      # pixels per index cell
    for scale, wanted in ((4, None), (2, 1), (1, 2)):
        for b in range(n):
            for i in range(gh // scale):
                for j in range(gw // scale):
                    if wanted is not None and indices[b, i * scale, j * scale] != wanted:
                        continue
                    top, left = ch * scale * i, cw * scale * j
                    pic[b, :, top, left:left + cw * scale] = -1
                    pic[b, :, top:top + ch * scale, left] = -1
    return pic


def line_mask(H, W, ind):
    """bool [H,W]: the line pixels of one image by the closed form; ind [gh,gw]"""
    gh, gw = ind.shape
    sh, sw = H // gh, W // gw
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    coarse = (y < 4 * sh * (gh // 4)) & (x < 4 * sw * (gw // 4)) & ((y % (4 * sh) == 0) | (x % (4 * sw) == 0))
    my, mx = np.minimum(2 * (y // (2 * sh)), gh - 1), np.minimum(2 * (x // (2 * sw)), gw - 1)
    medium = (y < 2 * sh * (gh // 2)) & (x < 2 * sw * (gw // 2)) & (ind[my, mx] == 1) & ((y % (2 * sh) == 0) | (x % (2 * sw) == 0))
    fy, fx = np.minimum(y // sh, gh - 1), np.minimum(x // sw, gw - 1)
    fine = (y < sh * gh) & (x < sw * gw) & (ind[fy, fx] == 2) & ((y % sh == 0) | (x % sw == 0))
    return coarse | medium | fine


def closed_form(images, indices):
    pic = images.copy()
    H, W = pic.shape[-2:]
    for b in range(indices.shape[0]):
        pic[b][:, line_mask(H, W, indices[b])] = -1
    return pic


def first_maximum(mc, mm, mf):
    """[B,h,w] int64 of 0/1/2: the first maximum over (up4(mc), up2(mm), mf), nonzero counting as 1; masks [B,1,.,.] or [B,.,.]"""
    B, h, w = mf.shape[0], mf.shape[-2], mf.shape[-1]
    c = np.repeat(np.repeat(mc.reshape(B, h // 4, w // 4) != 0, 4, 1), 4, 2)
    m = np.repeat(np.repeat(mm.reshape(B, h // 2, w // 2) != 0, 2, 1), 2, 2)
    f = mf.reshape(B, h, w) != 0
    stack = np.stack([c, m, f], axis=1).astype(np.int64)
    return stack.argmax(axis=1)                                    # numpy's argmax returns the first maximum


def random_partition(rng, B, H, W, p_coarse=0.35, p_medium=0.5):
    """a partition of B images of HxW as the router's int32 masks [B,1,.,.]: coarse cells, medium blocks among the rest, fine elsewhere"""
    mc = (rng.random((B, 1, H // 16, W // 16)) < p_coarse).astype(np.int32)
    free = 1 - np.repeat(np.repeat(mc, 2, 2), 2, 3)
    mm = ((rng.random((B, 1, H // 8, W // 8)) < p_medium) & (free == 1)).astype(np.int32)
    mf = (1 - np.repeat(np.repeat(mc, 4, 2), 4, 3)) * (1 - np.repeat(np.repeat(mm, 2, 2), 2, 3))
    return mc, mm, mf.astype(np.int32)


def to_unit(frames):
    """uint8 frames [B,H,W,3] -> fp32 [B,3,H,W]: byte / 255 (T.ToTensor())"""
    return (frames.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).astype(np.float32)


def to_frames(pic, line):
    """fp32 picture [B,3,H,W] + its line pixels (bool [B,H,W]) -> uint8 frames [B,H,W,3] by the conversion the header states:
    a line pixel is 1, any other trunc(255.0f * clamp(p, 0, 1)) with NaN -> 0"""
    p = pic.transpose(0, 2, 3, 1)
    with np.errstate(invalid="ignore"):
        c = np.where(p < 0, np.float32(0), np.where(p > 1, np.float32(1), p)).astype(np.float32)
        v = np.float32(255.0) * c
    fr = np.where(np.isnan(v), 0, np.nan_to_num(v, nan=0.0)).astype(np.uint8)
    fr[line] = 1
    return fr


def decode_pic(code):
    """the fixture's int16 coding of an fp32 picture (tests/golden/make_golden_partition.py: coded()): -1 = line, else byte b -> b / 255"""
    return np.where(code < 0, np.float32(-1), code.astype(np.float32) / np.float32(255)).astype(np.float32)


def geometry(H, W, tile):
    """(pad, tiles, groups) of the tiling driver for an HxW image"""
    pad, _ = highres.compute_padding(H, W)
    left, right, top, bottom = pad
    tiles = highres.tile_grid(H + top + bottom, W + left + right, tile)
    return pad, tiles, highres._shape_groups(tiles)


def tiled_expected(x, tile_inds, pad, tiles, draw=loop_draw):
    """the tiled map as the issue defines it: per tile, the drawer on that tile of the PADDED image with that tile's indices, then
    the unpad.  x [N,3,H,W] fp32; tile_inds[i] = [N,gh,gw] indices of tile i -> (picture [N,3,H,W], line pixels [N,H,W])"""
    left, right, top, bottom = pad
    N, _, H, W = x.shape
    padded = np.zeros((N, 3, H + top + bottom, W + left + right), dtype=x.dtype)
    padded[:, :, top:top + H, left:left + W] = x
    marks = np.zeros_like(padded)
    for (y, xx, th, tw), ind in zip(tiles, tile_inds):
        padded[:, :, y:y + th, xx:xx + tw] = draw(padded[:, :, y:y + th, xx:xx + tw], ind)
        marks[:, :, y:y + th, xx:xx + tw] = draw(np.zeros((N, 3, th, tw), dtype=x.dtype), ind)
    crop = lambda a: a[:, :, top:top + H, left:left + W]
    return crop(padded), crop(marks)[:, 0] == -1
