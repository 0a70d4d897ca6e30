#!/usr/bin/env python3
"""Golden fixture for the rate tables (tests/golden/rate.npz) from the REAL reference, CPU.

Runs only in the build container (needs the reference).  Config 1's CGIC with seeded weights compresses two 256x256 images
(oracle/content_families.py: an 8-bit noise image and a tie-heavy flat-with-edges one) at candidate ratios covering all seven
modes.  Recorded: the pixels (uint8), the entropy maps, the three encoder heads hooked at conv_out_coarse / conv_out /
conv_out_fine, quant_conv's weight and bias, the codebook, the usage counter behind the Huffman table, and per (image,
candidate) the real compress()'s indices and the size of every .bin file it wrote (0: not written).  Checked here: the indices
equal the per-head VQ (oracle) gathered through that candidate's masks -- the exactness argument of include/cgic_hip.h
section I -- and every file size is nbits // 8 + 2 (empty list: 0).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rate.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the harness shims, imports the reference)

from CGIC.tools.indices_coding import HuffmanCoding  # noqa: E402
from CGIC.tools.mask_coding import BinaryCoding  # noqa: E402
from oracle.content_families import families  # noqa: E402

CANDIDATES = [(0.1, 0.8), (0.1, 0.4), (0.3, 0.0), (0.2, 0.8), (0.0, 0.4), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.1, 0.0),
              (0.05, 0.55)]


def main():
    model = mg.build_model(0)
    fam = families(n=2, H=256, W=256, seed=11)
    imgs = [("noise8", fam["noise8"][0]), ("flat_edges", fam["flat_edges"][0])]
    freq = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)
    for i, v in enumerate(freq):
        model.quantize.embedding_counter[str(i)].data.fill_(float(v))
    hcoder, bcoder = HuffmanCoding(model.quantize.embedding_counter), BinaryCoding()
    htab = mg.orc.HuffmanTable(freq)
    lens = {s: len(c) for s, c in hcoder.codes.items()}
    cb = model.quantize.embedding.weight.detach().numpy().copy()
    qw = model.quant_conv.weight.detach().numpy().reshape(4, 4).copy()
    qb = model.quant_conv.bias.detach().numpy().copy()
    out = {"candidates": np.array(CANDIDATES, np.float64), "codebook": cb, "counter": freq, "qc_w": qw, "qc_b": qb,
           "names": np.array([n for n, _ in imgs])}
    enc = model.encoder
    for ii, (name, x_np) in enumerate(imgs):
        x = torch.from_numpy(x_np[None].copy())
        cap = {}
        hooks = [enc.conv_out_coarse.register_forward_hook(lambda m, i, o: cap.__setitem__("c", o.detach().clone())),
                 enc.conv_out.register_forward_hook(lambda m, i, o: cap.__setitem__("m", o.detach().clone())),
                 enc.conv_out_fine.register_forward_hook(lambda m, i, o: cap.__setitem__("f", o.detach().clone()))]
        with torch.no_grad():
            e8, e16 = model.entropy_calculation_p8(x), model.entropy_calculation_p16(x)
            model.encode(x)
        for h in hooks:
            h.remove()
        heads = {}
        with torch.no_grad():
            for g in "cmf":
                heads[g] = model.quant_conv(cap[g])
        vq = {g: mg.orc.vq(heads[g].numpy(), cb)[2].reshape(heads[g].shape[-2], heads[g].shape[-1]) for g in "cmf"}
        out[f"img{ii}_x"] = np.round(x_np.transpose(1, 2, 0) * 255.0).astype(np.uint8)          # [H,W,3]
        mg.check(np.array_equal(out[f"img{ii}_x"].transpose(2, 0, 1).astype(np.float32) / 255.0, x_np), "pixels are 8-bit")
        out[f"img{ii}_e8"], out[f"img{ii}_e16"] = e8.numpy(), e16.numpy()
        out[f"img{ii}_hc"], out[f"img{ii}_hm"], out[f"img{ii}_hf"] = cap["c"].numpy(), cap["m"].numpy(), cap["f"].numpy()
        modes = set()
        for ci, (c, m) in enumerate(CANDIDATES):
            enc.router_config["params"]["coarse_grain_ratio"] = c
            enc.router_config["params"]["medium_grain_ratio"] = m
            with torch.no_grad(), tempfile.TemporaryDirectory() as d:
                _, _, _, grain_mask, ind, _, mode = model.encode(x)
                model.decode = lambda q, mk: torch.zeros(1)          # (the decoder is not what is measured)
                _, bpp, _ = model.compress(x, d, hcoder, bcoder, False)
                del model.decode
                sizes = [os.path.getsize(os.path.join(d, n + ".bin")) if os.path.exists(os.path.join(d, n + ".bin")) else 0
                         for n in mg.orc.STREAM_NAMES]
            modes.add(mode)
            ind2 = ind.view(64, 64).numpy()
            mc, mm, mf = (t.numpy().reshape(t.shape[-2], t.shape[-1]) for t in grain_mask)
            # the exactness argument: the merged latent's indices are the per-head ones selected by the masks
            gathered = np.where(mf == 1, vq["f"], np.where(np.repeat(np.repeat(mm, 2, 0), 2, 1) == 1,
                                                           np.repeat(np.repeat(vq["m"], 2, 0), 2, 1),
                                                           np.repeat(np.repeat(vq["c"], 4, 0), 4, 1)))
            mg.check(np.array_equal(gathered, ind2), f"{name} candidate {ci}: per-head VQ gathered through the masks")
            # the byte formula
            on = mg.orc.mode_streams(mode)
            sel = (ind2[::4, ::4][mc == 1], ind2[::2, ::2][mm == 1], ind2[mf == 1])
            for s in range(3):
                want = 0 if not on[s] else (0 if sel[s].size == 0 else sum(lens[int(v)] for v in sel[s]) // 8 + 2)
                mg.check(sizes[s] == want, f"{name} candidate {ci}: stream {s} is {sizes[s]} bytes, formula {want}")
            for s, n in ((3, mc.size), (4, mm.size)):
                mg.check(sizes[s] == (n // 8 + 2 if on[s] else 0), f"{name} candidate {ci}: mask stream {s}")
            mg.check(sum(sizes) * 8 / (256 * 256) == bpp, f"{name} candidate {ci}: bpp")
            out[f"img{ii}_c{ci}_ind"] = ind2.astype(np.int16)
            out[f"img{ii}_c{ci}_sizes"] = np.array(sizes, np.int32)
            out[f"img{ii}_c{ci}_mode"] = np.int32(mode)
            print(f"  {name} ({c}, {m}) mode {mode}: sizes {sizes} bpp {bpp:.5f}")
        mg.check(modes == set(range(7)), f"{name}: candidates cover modes {sorted(modes)}")
    mg.save("rate", **out)


if __name__ == "__main__":
    main()
