#!/usr/bin/env python3
"""Golden vectors for the way OUT of the tiled path: blend weights, blend + normalise + clamp + unpad, uint8 frames.

Runs the REAL reference helpers (inference_high_resolution.py: _gaussian_weights :127-143, compute_padding :145-173,
nonoverlapping_grid_indices :112-125) and restates the body of its loop (:231-255) and write_images' conversion (:103) around
them on the CPU, with a seeded per-tile "decoder output" in place of model.compress.  Build container only (needs
/root/reference); the fixture holds data: the weights of four tile shapes, the per-tile inputs, the fp32 and the uint8 result.

The image is 776 x 8 (H x W): it pads to 784 x 16 (pad 4/4/4/4) and gives two real tiles, 768x16 and 16x16.

Before writing, the closed form cgic_paste_tiles evaluates (include/cgic_hip.h) is checked against the loop, value by value.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paste.py
"""
import math
import os
import sys
import types
from unittest.mock import MagicMock

# The reference takes exp from numpy (`from numpy import pi, exp, sqrt`), and numpy's float64 exp is its own AVX-512 kernel where the
# CPU has one and libm's exp everywhere else: the two differ by one ulp in about one value of twenty (160 of the 2912 factors of the
# extents 16, 32, 48, 592, 768; libm's are the correctly rounded ones but for 2), so the reference's weights depend on the machine it
# runs on.  The fixture pins the portable variant -- libm's, which is what cgic_tile_weights_host and highres.gaussian_weights
# (math.exp) evaluate -- by switching numpy's AVX-512 dispatch off before numpy is imported; that it took effect is asserted below.
os.environ["NPY_DISABLE_CPU_FEATURES"] = "AVX512F AVX512CD AVX512_SKX AVX512_CLX AVX512_CNL AVX512_ICL AVX512_SPR"

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

import inference_high_resolution as hr  # noqa: E402  (module-level code only defines functions/classes)
import torch.nn.functional as F  # noqa: E402

OUT = "paste.npz"
H, W = 776, 8
cpu = torch.device("cpu")
out = {"image_hw": np.array([H, W])}

for n_ in (16, 32, 48, 768):
    for mid_ in ((n_ - 1) / 2, n_ / 2):
        assert all(float(hr.exp(-(v - mid_) * (v - mid_) / (n_ * n_) / (2 * 0.01))) == math.exp(-(v - mid_) * (v - mid_) / (n_ * n_) / (2 * 0.01))
                   for v in range(n_)), "numpy's exp is not libm's in this process: the fixture would pin a machine-dependent variant"

# ---- the weights of four tile shapes (tile_width, tile_height) as the reference makes them
for tw, th in ((16, 16), (32, 16), (48, 32), (16, 768)):
    w = hr._gaussian_weights(tw, th, 1, cpu)
    assert w.dtype == torch.float64 and tuple(w.shape) == (1, 3, th, tw)
    assert torch.equal(w[0, 0], w[0, 1]) and torch.equal(w[0, 0], w[0, 2])
    out[f"weights_{tw}x{th}"] = w[0, 0].numpy().copy()

# ---- the loop, :226-255, with a seeded stand-in for the decoder
g = torch.Generator().manual_seed(9)
x = torch.zeros(1, 3, H, W)
h, w = x.shape[-2], x.shape[-1]
pad, unpad = hr.compute_padding(h, w, min_div=2 ** 4)
x_padded = F.pad(x, pad, mode="constant", value=0)
h_list, w_list, tile_height_size_list, tile_width_size_list = hr.nonoverlapping_grid_indices(x_padded)
assert pad == (4, 4, 4, 4) and tuple(x_padded.shape[-2:]) == (784, 16)
assert (h_list, w_list, tile_height_size_list, tile_width_size_list) == ([0, 768], [0], [768, 16], [16])
out["pad"] = np.array(pad)
out["h_list"], out["w_list"] = np.array(h_list), np.array(w_list)
out["tile_h"], out["tile_w"] = np.array(tile_height_size_list), np.array(tile_width_size_list)

x_rec = torch.zeros(x_padded.shape, device=x.device)
contributors = torch.zeros(x_padded.shape, device=x.device)
tiles = []
closed = torch.empty(x_padded.shape)
for i in range(len(h_list)):
    for j in range(len(w_list)):
        hi, wi = h_list[i], w_list[j]
        tile_hight_size, tile_width_size = tile_height_size_list[i], tile_width_size_list[j]
        tile_weights = hr._gaussian_weights(tile_width_size, tile_hight_size, 1, x_padded.device)
        x_tile_rec = torch.rand(1, 3, tile_hight_size, tile_width_size, generator=g) * 1.4 - 0.2          # the "decoder output"
        x_tile_rec[0, 0, 5, 5], x_tile_rec[0, 1, 6, 7], x_tile_rec[0, 2, 7, 9] = 0.0, 1.0, 128.0 / 255.0
        x_rec[:, :, hi:hi + tile_hight_size, wi:wi + tile_width_size] += x_tile_rec * tile_weights           # :248
        contributors[:, :, hi:hi + tile_hight_size, wi:wi + tile_width_size] += tile_weights                 # :249
        out[f"tile{len(tiles)}"] = x_tile_rec[0].numpy().copy()
        tiles.append(x_tile_rec)
        # the closed form: one tile per pixel
        wd = tile_weights.numpy()
        acc = (x_tile_rec.numpy().astype(np.float64) * wd).astype(np.float32)
        con = wd.astype(np.float32)
        closed[:, :, hi:hi + tile_hight_size, wi:wi + tile_width_size] = torch.from_numpy(np.clip(acc / con, np.float32(0), np.float32(1)))
x_rec /= contributors                                                                                        # :253
x_rec = x_rec.clamp(0, 1)                                                                                    # :254
assert x_rec.dtype == torch.float32
assert torch.equal(x_rec, closed), "the closed form is not the loop"
x_rec = F.pad(x_rec, unpad)                                                                                  # :255
assert tuple(x_rec.shape) == (1, 3, H, W)
images = (255 * x_rec.permute(0, 2, 3, 1).detach().cpu().numpy()).astype(np.uint8)                          # write_images, :103
assert np.array_equal(images, (np.float32(255.0) * F.pad(closed, unpad).permute(0, 2, 3, 1).numpy()).astype(np.uint8))
plain = torch.cat([t[0] for t in tiles], dim=1)[None].clamp(0, 1)
out["differs_from_plain_clamp"] = np.int64((F.pad(plain, unpad) != x_rec).sum())
assert out["differs_from_plain_clamp"] > 0, "the weights were expected not to cancel"
out["n_tiles"] = np.int32(len(tiles))
out["rec"] = x_rec.numpy().copy()
out["frames"] = images
np.savez_compressed(os.path.join(HERE, OUT), **out)
print("wrote", OUT, os.path.getsize(os.path.join(HERE, OUT)), "bytes;", int(out["differs_from_plain_clamp"]), "of", x_rec.numel(),
      "values differ from a plain clamp")
