#!/usr/bin/env python3
"""Golden fixture for the tie-heavy content families (tests/golden/ties.npz), from the REAL reference.

Runs only in the build container (needs /root/reference).  For small 8-bit images of every family of
oracle/content_families.py it runs the reference's own `Entropy(8)`, `Entropy(16)` (CGIC/models/model.py:433-483) and
`TripleGrainFixedEntropyRouter` (CGIC/modules/vqvae/RouterTriple.py) and stores inputs (uint8) and outputs.  Before writing
it requires that oracle/entropy_torch.py -- the torch-CPU restatement the GPU tests and bench.py use as "the reference's
arithmetic" on the GPU box -- reproduces the real class BIT FOR BIT (1 and 8 threads), on these images and on 256x256
ones, and that the oracle's router reproduces the real router's masks from those maps.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ties.py            # ties.npz, ties_host.npz, ties_batch.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ties.py batch      # ties_batch.npz only

ties_batch.npz: batches of B = 16 images of 256x256 -- one flattened segment beyond a router workgroup's LDS, so the GPU's
batch-global routing goes through router_big -- with the real router's masks over the flattened batch and per image.
"""
import os
import platform
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
pl = types.ModuleType("pytorch_lightning")
pl.LightningModule = torch.nn.Module
pl.LightningDataModule = object
sys.modules["pytorch_lightning"] = pl
tv = MagicMock()
sys.modules["torchvision"] = tv
sys.modules["torchvision.transforms"] = tv.transforms
torch.nn.Module.cuda = lambda self, device=None: self

from CGIC.models.model import Entropy  # noqa: E402
from CGIC.modules.vqvae.RouterTriple import TripleGrainFixedEntropyRouter  # noqa: E402

from oracle import cgic_oracle as orc  # noqa: E402
from oracle import entropy_torch as et  # noqa: E402
from oracle.content_families import families  # noqa: E402


def check(cond, msg):
    if not cond:
        raise SystemExit("MISMATCH: " + msg)


def cpu_vendor():
    """the CPU vendor of this host (/proc/cpuinfo vendor_id; "" elsewhere): torch's vectorised CPU exp / log round alike on one
    vendor's cores, not necessarily on another's"""
    try:
        with open("/proc/cpuinfo") as f:
            return next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("vendor_id")), "")
    except OSError:
        return ""


def main():
    out = {"torch_version": np.array(torch.__version__), "machine": np.array(platform.machine())}
    # 1. the restatement == the real class, bit for bit, on full-size images of every family, 1 and 8 threads
    for name, x in families(n=4, H=256, W=256, seed=21).items():
        xt = torch.from_numpy(x)
        for p in (8, 16):
            for nt in (8, 1):
                torch.set_num_threads(nt)
                check(torch.equal(Entropy(p)(xt), et.entropy_map(xt, p)), f"{name} p{p} threads {nt}: entropy_torch differs from the reference")
    torch.set_num_threads(8)
    # 2. the committed vectors: small images, reference outputs
    router = TripleGrainFixedEntropyRouter(0.1, 0.8)
    for name, x in families(n=2, H=96, W=128, seed=5).items():
        u8 = np.round(x * 255.0).astype(np.uint8)
        check(np.array_equal(u8.astype(np.float32) / 255.0, x), f"{name}: not exactly 8-bit")
        xt = torch.from_numpy(x)
        e8, e16 = Entropy(8)(xt), Entropy(16)(xt)
        check(torch.equal(e8, et.entropy_map(xt, 8)) and torch.equal(e16, et.entropy_map(xt, 16)), f"{name}: restatement")
        out[name + "_u8"] = u8
        out[name + "_e8"] = e8.numpy()
        out[name + "_e16"] = e16.numpy()
        for b in range(x.shape[0]):
            mask, _, _, mode = router(e16[b:b + 1], e8[b:b + 1])
            o = orc.router(e16[b:b + 1].numpy(), e8[b:b + 1].numpy(), 0.1, 0.8)
            check(o[4] == mode and all(np.array_equal(m.numpy(), q) for m, q in zip(mask, o[:3])), f"{name}[{b}]: oracle router")
            for k, m in zip("cmf", mask):
                out[f"{name}_{b}_m{k}"] = np.packbits(m.numpy().astype(np.uint8).reshape(-1))
        d8 = float(np.abs(orc.entropy(x, 8) - e8.numpy()).max())
        print(f"  {name}: distinct e8 values {len(np.unique(e8.numpy()))} of {e8.numel()}, C oracle max |diff| {d8:.2e}")
    # 3. (round 6) bands of realistic length for the GPU's pixels -> masks check: two 256x256 images per family and one smooth
    # 768x768 tile, per-image masks of the REAL router on the REAL Entropy maps, and the real router's batch-global masks
    # (the reference's encode() routes over the flattened batch: RouterTriple.py:21,40,52,63) of each pair.  Only inputs
    # (uint8) and masks (bits) are stored.  The masks must also follow from the correctly rounded restatement
    # (cgic_oracle_entropy_ref == the GPU's reference-order arithmetic, bit for bit): a fixture whose masks hang on MKL's
    # last-bit exp / log rounding could not be demanded of any other implementation.
    big = {name + "_256": x for name, x in families(n=2, H=256, W=256, seed=33).items()}
    big["smooth8_768"] = families(n=1, H=768, W=768, seed=11)["smooth8"]
    for name, x in big.items():
        u8 = np.round(x * 255.0).astype(np.uint8)
        check(np.array_equal(u8.astype(np.float32) / 255.0, x), f"{name}: not exactly 8-bit")
        xt = torch.from_numpy(x)
        e8, e16 = Entropy(8)(xt), Entropy(16)(xt)
        a8, a16 = orc.entropy_ref(x, 8), orc.entropy_ref(x, 16)
        out[name + "_u8"] = u8
        nb = x.shape[0]
        for b in list(range(nb)) + (["batch"] if nb > 1 else []):
            sl = slice(0, nb) if b == "batch" else slice(b, b + 1)
            mask, _, _, mode = router(e16[sl], e8[sl])
            o = orc.router(a16[sl], a8[sl], 0.1, 0.8)
            check(o[4] == mode and all(np.array_equal(m.numpy(), q) for m, q in zip(mask, o[:3])),
                  f"{name}[{b}]: the masks of the correctly rounded restatement differ from the real router's")
            for k, m in zip("cmf", mask):
                out[f"{name}_{b}_m{k}"] = np.packbits(m.numpy().astype(np.uint8).reshape(-1))
        t16 = np.sort(e16.numpy().reshape(-1))
        print(f"  {name}: distinct e16 {len(np.unique(t16))} of {t16.size}, "
              f"within 4e-6 of the coarse threshold: {int((np.abs(e16.numpy() - t16[max(round(t16.size / nb * 0.1) - 1, 0)]) < 4e-6).sum())}")
    path = os.path.join(HERE, "ties.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote ties.npz ({os.path.getsize(path)} bytes)")
    # the host whose torch build made (and reproduced) the maps above: the test's bit-for-bit branch runs on the same vendor only
    np.savez_compressed(os.path.join(HERE, "ties_host.npz"), cpu_vendor=np.array(cpu_vendor()))
    print(f"  wrote ties_host.npz (cpu_vendor {cpu_vendor()!r})")


BATCH_SETS = ("flat_edges", "blocky8")          # (smooth8 does not compress below the 1 MiB a committed file may have)
BATCH_RATIOS = ((0.1, 0.8), (0.0, 0.4))


def near_threshold(e16, e8, c, m):
    """entropies within 4e-6 of the threshold(s) the router draws at ratios (c, m) over the maps as given (RouterTriple.py:15-60)"""
    e16, e8 = e16.astype(np.float64), e8.astype(np.float64)
    near = 0
    keep8 = np.ones_like(e8)
    if c > 0:
        v = np.sort(e16.ravel())
        k = round(v.size * c)
        t = v[k - 1 if k else 0]
        near += int((np.abs(e16 - t) < 4e-6).sum())
        keep8 = 1.0 - np.repeat(np.repeat((e16 < t).astype(np.float64), 2, -2), 2, -1)
    if m > 0:
        v = np.sort((e8 * keep8).ravel())
        k = round(4 * e16.size * c + e8.size * m) if c > 0 else round(e8.size * m)
        t = v[k - 1 if k else 0]
        near += int((np.abs(e8 - t) < 4e-6).sum())
    return near


def batch_fixture():
    """4. (B = 16) the flattened batch beyond one workgroup's LDS: per set, 16 images of 256x256 (uint8), and for each ratio the REAL
    router's masks on the REAL Entropy maps over the flattened batch (the reference's encode(): RouterTriple.py:21,40,52,63) and
    per image, as packed bits of the whole [B,1,h,w] mask.  The oracle (entropy_ref -> router) must give the same masks, and every
    set must have entropies within 4e-6 of a threshold (the band decides something)."""
    router = {r: TripleGrainFixedEntropyRouter(*r) for r in BATCH_RATIOS}
    out = {"ratios": np.array(BATCH_RATIOS, np.float64), "sets": np.array(BATCH_SETS)}
    fam = families(n=16, H=256, W=256, seed=47)
    for name in BATCH_SETS:
        x = fam[name]
        u8 = np.round(x * 255.0).astype(np.uint8)
        check(np.array_equal(u8.astype(np.float32) / 255.0, x), f"{name}: not exactly 8-bit")
        xt = torch.from_numpy(x)
        e8, e16 = Entropy(8)(xt), Entropy(16)(xt)
        a8, a16 = orc.entropy_ref(x, 8), orc.entropy_ref(x, 16)
        out[name + "_u8"] = u8
        near = 0
        for ri, (c, m) in enumerate(BATCH_RATIOS):
            near_b = near_threshold(e16.numpy(), e8.numpy(), c, m)
            near_i = sum(near_threshold(e16[b].numpy(), e8[b].numpy(), c, m) for b in range(16))
            near += near_b + near_i
            for how in ("batch", "per"):
                sls = [slice(0, 16)] if how == "batch" else [slice(b, b + 1) for b in range(16)]
                ref, orac = [[], [], []], [[], [], []]
                for sl in sls:
                    mask, _, _, mode = router[(c, m)](e16[sl], e8[sl])
                    o = orc.router(a16[sl], a8[sl], c, m)
                    check(o[4] == mode, f"{name} {how} ({c}, {m}): mode")
                    for k in range(3):
                        ref[k].append(mask[k].numpy())
                        orac[k].append(o[k])
                for k, g in enumerate("cmf"):
                    r = np.concatenate(ref[k])
                    check(np.array_equal(r, np.concatenate(orac[k])),
                          f"{name} {how} ({c}, {m}) m{g}: the oracle's masks differ from the real router's on the real maps")
                    out[f"{name}_r{ri}_{how}_m{g}"] = np.packbits(r.astype(np.uint8).reshape(-1))
            out[f"{name}_r{ri}_mode"] = np.array(mode)
            print(f"  {name} ({c}, {m}): within 4e-6 of a threshold: {near_b} batch-global, {near_i} per image")
        check(near > 0, f"{name}: no entropy within 4e-6 of a threshold")
    path = os.path.join(HERE, "ties_batch.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote ties_batch.npz ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    if sys.argv[1:] != ["batch"]:
        main()
    batch_fixture()
