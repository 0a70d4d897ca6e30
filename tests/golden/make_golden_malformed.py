#!/usr/bin/env python3
"""Generate tests/golden/malformed.npz: what the REAL reference makes of every malformed stream of tests/malformed_ref.py.

Runs only where the reference tree exists (like make_golden_contract.py, with the same shims; nothing from it is copied here -- the
fixture is data: the mutants' bytes and the reference's verdict on them).

Single streams: the real HuffmanCoding.decompress_string / BinaryCoding.decompress_string on the mutated bytes.
Whole images: the real CGIC.compress, whose coders are arguments: thin wrappers whose `compress` writes the mutant's bytes (or no
file at all) and whose `decompress_string` is the real one; `encode`, `decode` and `quantize.embedding` of the instance are
stand-ins that supply ind, masks and mode and capture `ind_decompress` and `grain_mask_decompress`.  Recorded per mutant: the bytes,
mode, h, w, whether the call raised and the exception's type name, else the decoded index grid and the three masks.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_malformed.py
"""
import os
import sys
import tempfile
import types
from unittest.mock import MagicMock

import numpy as np
import torch
import yaml

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# ---- shims -------------------------------------------
pl = types.ModuleType("pytorch_lightning")
pl.LightningModule = torch.nn.Module
pl.LightningDataModule = object
sys.modules["pytorch_lightning"] = pl
tv = MagicMock()
for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional", "torchvision.utils"):
    sys.modules[n] = tv
torch.nn.Module.cuda = lambda self, device=None: self

from CGIC.models.model import CGIC  # noqa: E402
from CGIC.tools.indices_coding import HuffmanCoding as RefHuffman  # noqa: E402
from CGIC.tools.mask_coding import BinaryCoding as RefBinary  # noqa: E402

import malformed_ref as mr  # noqa: E402
from oracle import cgic_oracle as orc  # noqa: E402


class MutantCoder:
    """a coder whose compress writes the mutant's bytes under the file name it is given, or no file when the mutant has none"""

    def __init__(self, real, streams):
        self.real, self.streams = real, streams

    def compress(self, info, output_path):
        name = os.path.basename(output_path)[:-len(".bin")]
        if name in self.streams:
            with open(output_path, "wb") as f:
                f.write(self.streams[name])
        return output_path

    def decompress_string(self, path):
        return self.real.decompress_string(path)


def run_image(model, huff, binary, m, base):
    """the real CGIC.compress on one mutant -> (raised, type name, ind, [mask_c, mask_m, mask_f])"""
    got = {}
    ind = torch.from_numpy(base.ind).view(1, m.h, m.w)
    masks = [torch.from_numpy(a.astype(np.int64)).view(1, 1, *a.shape) for a in base.masks]
    model.encode = lambda x: (torch.zeros(1, 4, m.h, m.w), None, None, masks, ind.flatten(), None, m.mode)

    def embedding(flat):
        got["ind"] = flat.detach().clone()
        return torch.zeros(flat.numel(), 4)

    def decode(quant, grain_mask):
        got["masks"] = [g.detach().clone() for g in grain_mask]
        return quant

    model.quantize.embedding = embedding
    model.decode = decode
    with tempfile.TemporaryDirectory() as d:
        try:
            model.compress(torch.zeros(1, 3, 4 * m.h, 4 * m.w), d, MutantCoder(huff, m.streams), MutantCoder(binary, m.streams), False)
        except Exception as e:  # noqa: BLE001  (the verdict IS the exception)
            return True, type(e).__name__, None, None
    return False, "", got["ind"].reshape(m.h, m.w).to(torch.float64).numpy(), [g.to(torch.float64).numpy().ravel() for g in got["masks"]]


def pack(blobs):
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    return np.frombuffer(b"".join(blobs), np.uint8), off


def main():
    coders = np.load(os.path.join(HERE, "coders.npz"))
    freq, order = coders["zipf_freq"], coders["zipf_order"]
    pd = torch.nn.ParameterDict({str(int(k)): torch.nn.Parameter(torch.tensor([float(freq[int(k)])])) for k in order}).requires_grad_(False)
    huff, binary = RefHuffman(pd), RefBinary()
    htab = orc.HuffmanTable(freq)
    assert all(huff.codes[s] == htab.code_str(s) for s in range(htab.n)), "the oracle's table is not the reference's"

    params = yaml.safe_load(open(os.path.join(REF, "configs", "config_inference.yaml")))["model"]["params"]
    params["ckpt_path"] = None
    params["lossconfig"] = None
    torch.manual_seed(0)
    model = CGIC(**params).eval()
    del model.quantize.embedding                      # (a registered submodule: a plain function cannot be assigned over it)

    out, names, modes, hw, present, blobs, raised, exc, inds, maskv = {}, [], [], [], [], [], [], [], [], []
    ss_names, ss_kind, ss_blobs, ss_none, ss_syms = [], [], [], [], []
    for (h, w), seed in zip(mr.FIXTURE_GRIDS, mr.FIXTURE_SEEDS):
        bases = {b.mode: b for b in mr.base_images(orc, htab, h, w, seed)}
        for m in mr.catalogue(orc, htab, h, w, seed):
            r, e, ind, masks = run_image(model, huff, binary, m, bases[m.mode])
            names.append(f"{h}x{w}-{m.name}"); modes.append(m.mode); hw.append((h, w))
            present.append([n in m.streams for n in orc.STREAM_NAMES])
            blobs += [m.streams.get(n, b"") for n in orc.STREAM_NAMES]
            raised.append(r); exc.append(e)
            if not r:
                assert np.array_equal(ind, np.round(ind)) and np.abs(ind).max() < 2 ** 15
                inds.append(ind.astype(np.int16).ravel())
                maskv.append(np.concatenate(masks).astype(np.int8))
        for name, kind, data in mr.single_stream_mutants(orc, htab, h, w, seed):
            with tempfile.TemporaryDirectory() as d:
                p = os.path.join(d, "s.bin")
                with open(p, "wb") as f:
                    f.write(data)
                dec = (huff if kind == "huffman" else binary).decompress_string(p)
            ss_names.append(f"{h}x{w}-{name}"); ss_kind.append(kind); ss_blobs.append(data)
            ss_none.append(dec is None); ss_syms.append(np.asarray([] if dec is None else dec, np.int16))
    out["names"], out["mode"], out["hw"] = np.array(names), np.array(modes, np.int8), np.array(hw, np.int16)
    out["present"] = np.array(present, bool)
    out["bytes"], out["bytes_off"] = pack(blobs)
    out["raised"], out["exc"] = np.array(raised, bool), np.array(exc)
    out["ind"], out["masks"] = np.concatenate(inds), np.concatenate(maskv)
    out["ss_names"], out["ss_kind"], out["ss_none"] = np.array(ss_names), np.array(ss_kind), np.array(ss_none, bool)
    out["ss_bytes"], out["ss_bytes_off"] = pack(ss_blobs)
    out["ss_syms"] = np.concatenate(ss_syms)
    out["ss_syms_off"] = np.cumsum([0] + [len(s) for s in ss_syms]).astype(np.int64)
    path = os.path.join(HERE, "malformed.npz")
    np.savez_compressed(path, **out)
    kinds = {}
    for n, r, e in zip(names, raised, exc):
        kinds[e if r else "accepted"] = kinds.get(e if r else "accepted", 0) + 1
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(names)} images {kinds}, {len(ss_names)} single streams")


if __name__ == "__main__":
    main()
