#!/usr/bin/env python3
"""Golden vectors for the partition map: the pictures of the REAL draw_triple_grain_256res (CGIC/modules/draw.py:78-119).

Runs the real drawer on masks of the REAL TripleGrainFixedEntropyRouter (CGIC/modules/vqvae/RouterTriple.py) in all seven routing
modes, on arbitrary indices over a ragged grid, on the malformed [B,1,h] `grain_indices` the stock encoder makes
(vqvae_blocks.py:357-359), and tile by tile on two padded images cut with the real compute_padding / nonoverlapping_grid_indices
(inference_high_resolution.py:112-125,:145-173), plus write_images' uint8 conversion (:103) of every picture.  Build container only
(needs /root/reference); the fixture holds data: inputs, masks, indices and the reference's pictures (fp32 pictures as int16 codes, see coded()).

The images are seeded byte patterns divided by 255 (what T.ToTensor() gives), so that the fp32 and the uint8 form of an input are
one image and the fixture compresses.

Before writing, the closed form cgic_partition_map evaluates (include/cgic_hip.h) is checked against every recorded picture, value by
value; a line pixel is checked to convert to byte 1 and the 256-byte round trip to be the identity.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_partition.py
"""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
pl = types.ModuleType("pytorch_lightning")
pl.LightningModule = torch.nn.Module
pl.LightningDataModule = object
sys.modules["pytorch_lightning"] = pl
for name in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.utils",
             "omegaconf", "PIL", "PIL.Image"):
    sys.modules.setdefault(name, MagicMock())
torch.nn.Module.cuda = lambda self, device=None: self

from CGIC.modules.draw import draw_triple_grain_256res  # noqa: E402
from CGIC.modules.vqvae.RouterTriple import TripleGrainFixedEntropyRouter  # noqa: E402
import inference_high_resolution as hr  # noqa: E402  (module-level code only defines functions/classes)
import torch.nn.functional as F  # noqa: E402

OUT = "partition.npz"
SHAPES = [(1, 16, 16), (2, 32, 48), (1, 64, 32)]
RATIOS = [(0.25, 0.5), (0, 0.5), (0.5, 0), (0.3, 0.7), (1, 0), (0, 1), (0, 0)]
out = {"shapes": np.array(SHAPES), "ratios": np.array(RATIOS, dtype=np.float64)}


def image_bytes(B, H, W, seed):
    """uint8 frames [B,H,W,3]: a seeded pattern of sixteen byte levels, 0 and 255 among them (compresses; no two rows or columns alike)"""
    g = np.random.default_rng(seed)
    b, y, x, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    v = ((y * 5 + x * 3 + c * 7 + b * 11 + (y * x) // 7) % 16) * 17
    v[g.random(v.shape) < 0.005] = 128
    return v.astype(np.uint8)


def to_tensor(frames):
    """T.ToTensor() on every frame: byte / 255 in float32, [B,3,H,W]"""
    return torch.from_numpy(frames).permute(0, 3, 1, 2).float().div(255).contiguous()


def first_maximum(mask):
    """[B,h,w] int64: argmax over (up4(coarse), up2(medium), fine) -- what the comment at vqvae_blocks.py:358 means"""
    up = lambda m, k: m.repeat_interleave(k, -2).repeat_interleave(k, -1)
    gate = torch.stack([up(mask[0][:, 0], 4), up(mask[1][:, 0], 2), mask[2][:, 0]], dim=1)
    return gate.argmax(dim=1)


def closed_form(images, indices):
    """the header's closed form, vectorised: images [B,3,H,W] float32 numpy, indices [B,gh,gw] -> the picture"""
    B, _, H, W = images.shape
    _, gh, gw = indices.shape
    sh, sw = H // gh, W // gw
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    res = images.copy()
    for b in range(indices.shape[0]):
        ind = indices[b]
        coarse = (y < 4 * sh * (gh // 4)) & (x < 4 * sw * (gw // 4)) & ((y % (4 * sh) == 0) | (x % (4 * sw) == 0))
        inm = (y < 2 * sh * (gh // 2)) & (x < 2 * sw * (gw // 2))
        my, mx = np.minimum(2 * (y // (2 * sh)), gh - 1), np.minimum(2 * (x // (2 * sw)), gw - 1)
        medium = inm & (ind[my, mx] == 1) & ((y % (2 * sh) == 0) | (x % (2 * sw) == 0))
        inf_ = (y < sh * gh) & (x < sw * gw)
        fy, fx = np.minimum(y // sh, gh - 1), np.minimum(x // sw, gw - 1)
        fine = inf_ & (ind[fy, fx] == 2) & ((y % sh == 0) | (x % sw == 0))
        res[b][:, coarse | medium | fine] = -1
    return res


def coded(pic, frames):
    """a picture as int16 [B,3,H,W]: -1 for a line pixel, else the byte b whose b / 255 the value is -- lossless (asserted), and it
    compresses where float32 does not; tests decode it with np.where(c < 0, -1, c / 255) in float32"""
    p = pic.numpy()
    code = np.where(p == -1, -1, frames.transpose(0, 3, 1, 2).astype(np.int16)).astype(np.int16)
    back = np.where(code < 0, np.float32(-1), code.astype(np.float32) / np.float32(255))
    assert back.dtype == np.float32 and np.array_equal(back, p), "the int16 coding of the picture is not lossless"
    return code


def frames_of(pic):
    """write_images' conversion, inference_high_resolution.py:103"""
    return (255 * pic.permute(0, 2, 3, 1).detach().cpu().numpy()).astype(np.uint8)


def record(key, frames, indices):
    """draw with the REAL function, check the closed form and the byte conversion, record picture + frames"""
    x = to_tensor(frames)
    pic = draw_triple_grain_256res(x.clone(), indices)
    assert pic.dtype == torch.float32 and pic.shape == x.shape
    want = closed_form(x.numpy(), indices.numpy())
    assert np.array_equal(pic.numpy(), want), f"{key}: the closed form is not the reference's picture"
    fr = frames_of(pic)
    line = (pic.numpy() == -1).transpose(0, 2, 3, 1)
    assert line.any() or indices.shape[1] < 4
    assert np.all(fr[line] == 1), "a line pixel does not convert to byte 1 on this machine"
    assert np.array_equal(fr[~line], frames[~line]), "the byte round trip is not the identity"
    out[f"{key}_pic"] = coded(pic, frames)
    out[f"{key}_frames"] = fr
    return pic


# the 256-byte round trip of write_images on ToTensor's values
allb = np.arange(256, dtype=np.uint8)
assert np.array_equal((255 * (torch.from_numpy(allb).float().div(255)).numpy()).astype(np.uint8), allb)
assert (255 * np.float32(-1)).astype(np.uint8) == 1

# ---- draws: three batch shapes x the seven routing modes -------------------------------------------------------------
modes_seen = set()
for si, (B, H, W) in enumerate(SHAPES):
    frames = image_bytes(B, H, W, 100 + si)
    out[f"s{si}_x"] = frames
    g = torch.Generator().manual_seed(200 + si)
    e16, e8 = torch.rand(B, H // 16, W // 16, generator=g), torch.rand(B, H // 8, W // 8, generator=g)
    for ri, (rc, rm) in enumerate(RATIOS):
        mask, gate, _, mode = TripleGrainFixedEntropyRouter(rc, rm)(e16, e8)
        modes_seen.add(mode)
        assert all(m.dtype == torch.int32 for m in mask)
        ind = first_maximum(mask)
        key = f"s{si}_r{ri}"
        out[f"{key}_mc"], out[f"{key}_mm"], out[f"{key}_mf"] = (m.numpy().astype(np.int8) for m in mask)
        out[f"{key}_ind"] = ind.numpy().astype(np.int8)
        record(key, frames, ind)
        if (B, H, W) == (2, 32, 48) and ri == 0:
            # ---- the malformed case: the gate pushed through the encoder's permute + argmax (vqvae_blocks.py:357-359)
            bad = gate.permute(0, 3, 1, 2).argmax(dim=1)
            assert tuple(bad.shape) == (2, 1, 8) and int(bad.max()) > 2
            out["malformed_ind"] = bad.numpy().astype(np.int64)
            record("malformed", frames, bad)
assert modes_seen == set(range(7)), modes_seen

# ---- arbitrary indices on a ragged image -----------------------------------------------------------------------------
frames = image_bytes(1, 27, 41, 300)
ind = torch.randint(-1, 4, (1, 6, 10), generator=torch.Generator().manual_seed(301))
out["ragged_x"], out["ragged_ind"] = frames, ind.numpy().astype(np.int64)
record("ragged", frames, ind)

# ---- two tiled images: per tile the real drawer on that tile of the padded image, then the unpad ------------------------
for name, (H, W, tile) in (("t0", (40, 56, 32)), ("t1", (17, 33, 16))):
    frames = image_bytes(1, H, W, 400 + tile)
    x = to_tensor(frames)
    pad, unpad = hr.compute_padding(H, W, min_div=2 ** 4)
    x_padded = F.pad(x, pad, mode="constant", value=0)
    # the real grid function has its 768 built in: it is asked about an image 768 / tile times as large and its answer scaled back
    k = 768 // tile
    ph, pw = x_padded.shape[-2:]
    h_list, w_list, th_list, tw_list = hr.nonoverlapping_grid_indices(torch.empty(1, 3, ph * k, pw * k, device="meta"))
    assert all(v % k == 0 for v in h_list + w_list + th_list + tw_list)
    h_list, w_list, th_list, tw_list = ([v // k for v in l] for l in (h_list, w_list, th_list, tw_list))
    g = torch.Generator().manual_seed(500 + tile)
    pic = x_padded.clone()
    n = 0
    for i, hi in enumerate(h_list):
        for j, wi in enumerate(w_list):
            th, tw = th_list[i], tw_list[j]
            e16, e8 = torch.rand(1, th // 16, tw // 16, generator=g), torch.rand(1, th // 8, tw // 8, generator=g)
            mask, _, _, _ = TripleGrainFixedEntropyRouter(0.25, 0.5)(e16, e8)
            part = draw_triple_grain_256res(x_padded[:, :, hi:hi + th, wi:wi + tw].clone(), first_maximum(mask))
            assert np.array_equal(part.numpy(), closed_form(x_padded[:, :, hi:hi + th, wi:wi + tw].numpy(), first_maximum(mask).numpy()))
            pic[:, :, hi:hi + th, wi:wi + tw] = part
            out[f"{name}_tile{n}"] = np.array([hi, wi, th, tw])
            out[f"{name}_tile{n}_mc"], out[f"{name}_tile{n}_mm"], out[f"{name}_tile{n}_mf"] = (m.numpy().astype(np.int8) for m in mask)
            n += 1
    pic = F.pad(pic, unpad)
    assert tuple(pic.shape) == (1, 3, H, W)
    out[f"{name}_x"], out[f"{name}_hw_tile"], out[f"{name}_pad"], out[f"{name}_ntiles"] = frames, np.array([H, W, tile]), np.array(pad), np.int32(n)
    out[f"{name}_pic"], out[f"{name}_frames"] = coded(pic, frames), frames_of(pic)
    line = (pic.numpy() == -1).transpose(0, 2, 3, 1)
    assert np.all(out[f"{name}_frames"][line] == 1) and np.array_equal(out[f"{name}_frames"][~line], frames[~line])

path = os.path.join(HERE, OUT)
np.savez_compressed(path, **out)
print("wrote", OUT, os.path.getsize(path), "bytes,", len(out), "arrays")
assert os.path.getsize(path) < 150 * 1024
