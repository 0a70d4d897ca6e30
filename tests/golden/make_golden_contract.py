#!/usr/bin/env python3
"""Generate tests/golden/cgic_contract.npz: the attribute contract of the REAL reference `CGIC` model that install() relies on.

Runs only where the reference tree exists (like make_golden.py, with the same shims; nothing from it is copied here -- the
fixture is data: state_dict key names and shapes, a few attribute values, the quantiser's initial weights and counters, the
router config, and the Huffman codes the reference builds from those counters).  Before writing, install() is run on the real
model and checked on the spot; a failure aborts, so a committed fixture implies "install() held on the real class".
tests/test_reference_contract.py rebuilds a CGIC-shaped module tree from the fixture and checks install() against it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_contract.py
"""
import json
import os
import sys
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
from CGIC.util import instantiate_from_config  # noqa: E402
import control_gic_amd as cg  # noqa: E402


def main():
    params = yaml.safe_load(open(os.path.join(REF, "configs", "config_inference.yaml")))["model"]["params"]
    params["ckpt_path"] = None
    params["lossconfig"] = None
    torch.manual_seed(0)
    model = CGIC(**params).eval()

    q = model.quantize
    sd = model.state_dict()
    names = list(sd)
    params_of = {n for n, _ in model.named_parameters()}
    shapes = np.full((len(names), 4), -1, np.int64)
    for i, n in enumerate(names):
        shapes[i, :sd[n].dim()] = sd[n].shape
    q.embedding_counter["7"].data.fill_(42.0)
    counter_keys = list(q.embedding_counter.keys())
    ref_codes = RefHuffman({k: q.embedding_counter[k] for k in q.embedding_counter}).codes
    assert all(isinstance(k, int) for k in ref_codes)
    dec = model.decoder
    pools = {}
    for name in ("avgpool_layer1", "avgpool_layer2"):
        m = getattr(dec, name)
        pools[name] = {"type": type(m).__name__, "kernel_size": m.kernel_size, "stride": m.stride, "padding": m.padding}
    facts = {
        "quantize_type": type(q).__name__, "n_e": q.n_e, "e_dim": q.e_dim, "beta": q.beta, "legacy": q.legacy,
        "router_config": model.encoder.router_config,
        "entropy_types": [type(model.entropy_calculation_p8).__name__, type(model.entropy_calculation_p16).__name__],
        "convs": {n: {"type": type(getattr(model, n)).__name__, "in_channels": getattr(model, n).in_channels,
                      "out_channels": getattr(model, n).out_channels, "kernel_size": list(getattr(model, n).kernel_size),
                      "bias": getattr(model, n).bias is not None} for n in ("quant_conv", "post_quant_conv")},
        "decoder_pools": pools,
        "callables": [n for n in ("encode", "decode", "compress") if callable(getattr(model, n, None))],
    }
    facts = json.dumps(facts)                                  # before install(), which rewrites router_config in place
    weight = q.embedding.weight.detach().numpy().copy()
    counter = np.array([float(q.embedding_counter[k].item()) for k in counter_keys], np.float64)

    # ---- install() on the real model, checked on the spot (what the test restates on the fixture's module tree)
    keys = {k: tuple(v.shape) for k, v in sd.items()}
    cg.install(model)
    assert isinstance(model.quantize, cg.VectorQuantize2) and isinstance(model.entropy_calculation_p8, cg.Entropy)
    assert model.encoder.router_config["target"] == "control_gic_amd.router.TripleGrainFixedEntropyRouter"
    r = instantiate_from_config(model.encoder.router_config)
    assert isinstance(r, cg.TripleGrainFixedEntropyRouter) and r.per_image is False
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == keys
    assert np.array_equal(model.quantize.embedding.weight.detach().numpy(), weight)
    assert cg.HuffmanCoding(model.quantize.embedding_counter).codes == ref_codes

    code_keys = np.array(sorted(ref_codes), np.int64)
    path = os.path.join(HERE, "cgic_contract.npz")
    np.savez_compressed(path, facts=np.array(facts), sd_names=np.array(names),
                        sd_shapes=shapes, sd_is_param=np.array([n in params_of for n in names]),
                        quantize_weight=weight, counter_keys=np.array(counter_keys), counter=counter,
                        code_keys=code_keys, codes=np.array([ref_codes[k] for k in code_keys]))
    print(f"wrote {path} ({os.path.getsize(path)} bytes): {len(names)} state_dict entries")


if __name__ == "__main__":
    main()
