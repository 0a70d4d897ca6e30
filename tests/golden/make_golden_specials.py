#!/usr/bin/env python3
"""Golden fixture for entropy maps that hold NaN, +-Inf, negatives, signed zeros and denormals (tests/golden/router_specials.npz),
from the REAL reference router.

Runs only in the build container (needs /root/reference).  For every shape and map class of tests/specials_ref.py it runs the
reference's own `TripleGrainFixedEntropyRouter` (CGIC/modules/vqvae/RouterTriple.py) at ratio pairs of all seven modes, over the
flattened batch and as B separate B = 1 calls, and stores the maps (float32, bit for bit) and the masks (one packed bit string per
pair of maps; specials_ref.fixture_masks unpacks it).  Before it writes it requires that the oracle's router
(oracle/cgic_oracle.c) gives the same masks and mode everywhere.  Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_specials.py
"""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pl = types.ModuleType("pytorch_lightning")
pl.LightningModule = torch.nn.Module
pl.LightningDataModule = object
sys.modules["pytorch_lightning"] = pl
tv = MagicMock()
sys.modules["torchvision"] = tv
sys.modules["torchvision.transforms"] = tv.transforms

from CGIC.modules.vqvae.RouterTriple import TripleGrainFixedEntropyRouter  # noqa: E402

import specials_ref as sr  # noqa: E402
from oracle import cgic_oracle as orc  # noqa: E402


def check(cond, msg):
    if not cond:
        raise SystemExit("MISMATCH: " + msg)


def main():
    out = {"ratios": np.array(sr.RATIOS, np.float64), "shapes": np.array(sr.SHAPES, np.int64), "classes": np.array(sr.CLASSES)}
    routers = [TripleGrainFixedEntropyRouter(c, m) for c, m in sr.RATIOS]
    modes = set()
    for si, (B, h16, w16) in enumerate(sr.SHAPES):
        for ci, cls in enumerate(sr.CLASSES):
            e16, e8 = sr.special_maps(B, h16, w16, cls, seed=1000 * si + ci)
            key = f"s{si}_{cls}"
            out[key + "_e16"], out[key + "_e8"] = e16, e8
            t16, t8 = torch.from_numpy(e16), torch.from_numpy(e8)
            bits = []                                  # ratio by ratio: flattened-batch mc, mm, mf, then per-image mc, mm, mf
            for ri, (c, m) in enumerate(sr.RATIOS):
                for how in ("batch", "per"):
                    sls = [slice(0, B)] if how == "batch" else [slice(b, b + 1) for b in range(B)]
                    ref = [[], [], []]
                    for sl in sls:
                        mask, _, _, mode = routers[ri](t16[sl], t8[sl])
                        for k in range(3):
                            ref[k].append(mask[k].numpy())
                    o = orc.router(e16, e8, c, m, per_image=how == "per")
                    check(o[4] == mode, f"{key} ({c}, {m}) {how}: mode {o[4]} != {mode}")
                    for k, g in enumerate("cmf"):
                        r = np.concatenate(ref[k])
                        check(np.array_equal(r, o[k]), f"{key} ({c}, {m}) {how} m{g}: the oracle's masks differ from the real router's")
                        check(set(np.unique(r)) <= {0, 1}, f"{key}: mask values")
                        bits.append(r.astype(np.uint8).reshape(-1))
                out[f"r{ri}_mode"] = np.array(mode)
                modes.add(mode)
            out[key + "_masks"] = np.packbits(np.concatenate(bits))
    check(modes == set(range(7)), f"modes {sorted(modes)}")
    path = os.path.join(HERE, "router_specials.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote router_specials.npz ({os.path.getsize(path)} bytes, {len(out)} arrays)")
    check(os.path.getsize(path) < 100 * 1024, "the fixture must stay under 100 KB")


if __name__ == "__main__":
    main()
