#!/usr/bin/env python3
"""Writes tests/golden/ema.npz from the REAL LitEma (CGIC/models/ema.py), run on the CPU.  Data only:

  * for a small seeded module (a conv, a GroupNorm, a Linear with a one-element bias and a frozen parameter), both use_num_upates
    settings and STEPS steps: the initial parameters, the parameters at each step, the shadows after each step, num_updates after each
    step, and the state_dict keys.  With use_num_upates the run starts at num_updates = START, so that the steps straddle the
    crossing of (1 + n) / (10 + n) with the decay 0.9999 (n = 89 990 / 89 991); a second counted run starts at 0;
  * the trainable-tensor shapes of the real Encoder, Decoder, quantiser and the two 1x1 convolutions at the training config
    (configs/config_train.yaml): the tensors the five LitEma modules of CGIC.__init__ (model.py:74-78) hold, in their order.

While it writes, it holds tests/ema_ref.py's restatement to the class, bit for bit.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ema.py
"""
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (applies the harness shims, puts the reference on the path)
import ema_ref as eref    # noqa: E402

from CGIC.models.ema import LitEma  # noqa: E402

STEPS = 5
START = 89988          # counted run "cross": num_updates before its first step
DECAY = 0.9999


class Small(torch.nn.Module):
    """the fixture's module; tests/test_ema_host.py builds the same one (only names, shapes and requires_grad matter: the values
    come from the file)"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 3)
        self.norm = torch.nn.GroupNorm(1, 5)
        self.head = torch.nn.Linear(5, 1)
        self.frozen = torch.nn.Parameter(torch.zeros(7), requires_grad=False)


def run(out, tag, use_num_upates, start):
    torch.manual_seed(7)
    m = Small()
    rng = np.random.default_rng(11)
    ema = LitEma(m, DECAY, use_num_upates=use_num_upates)
    if start:
        ema.num_updates.fill_(start)
    names = [k for k, p in m.named_parameters()]
    out[tag + "/names"] = np.array(names)
    out[tag + "/trainable"] = np.array([int(p.requires_grad) for p in m.parameters()], np.int8)
    out[tag + "/keys"] = np.array(list(ema.state_dict().keys()))
    out[tag + "/start"] = np.array(int(ema.num_updates), np.int32)
    for k, p in m.named_parameters():
        out[f"{tag}/init/{k}"] = p.detach().numpy().copy()
    mine = {k: p.detach().clone() for k, p in m.named_parameters() if p.requires_grad}
    n = int(ema.num_updates)
    for step in range(STEPS):
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.add_(torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)) * 0.05)
                out[f"{tag}/param{step}/{k}"] = p.detach().numpy().copy()
        ema(m)
        keys = [k for k in mine]
        new, n = eref.update([mine[k] for k in keys], [dict(m.named_parameters())[k].detach() for k in keys], DECAY, n if use_num_upates else None)
        n = n if use_num_upates else -1
        mine = dict(zip(keys, new))
        for k in keys:
            s = dict(ema.named_buffers())[ema.m_name2s_name[k]]
            mg.check(torch.equal(eref.bits(s), eref.bits(mine[k])), f"ema_ref.update == LitEma.forward, {tag} step {step} {k}")
            out[f"{tag}/shadow{step}/{k}"] = s.detach().numpy().copy()
        mg.check(int(ema.num_updates) == n, "num_updates")
        out[f"{tag}/num_updates{step}"] = np.array(int(ema.num_updates), np.int32)
    for k, v in ema.state_dict().items():
        out[f"{tag}/sd/{k}"] = v.numpy().copy()
    print(f"  {tag}: num_updates {int(out[tag + '/start'])} -> {int(ema.num_updates)}, {len(mine)} trainable tensors")


def model_shapes(out):
    from CGIC.modules.vqvae.vqvae_blocks import Encoder
    from CGIC.modules.vqvae.decoder import Decoder
    from CGIC.modules.vqvae.quantize import VectorQuantize2 as VectorQuantizer          # (model.py:11's import)
    params = yaml.safe_load(open(os.path.join(mg.REF, "configs/config_train.yaml")))["model"]["params"]
    dd = params["ddconfig"]
    torch.manual_seed(0)
    parts = (("encoder", Encoder(**dd)), ("decoder", Decoder(zq_ch=params["embed_dim"], **dd)),
             ("quantize", VectorQuantizer(params["n_embed"], params["embed_dim"], beta=0.25)),
             ("quant_conv", torch.nn.Conv2d(dd["z_channels"], params["embed_dim"], 1)),
             ("post_quant_conv", torch.nn.Conv2d(params["embed_dim"], dd["z_channels"], 1)))
    numels, owner, shapes = [], [], []
    for i, (name, m) in enumerate(parts):
        ema = LitEma(m, DECAY)
        for k, p in m.named_parameters():
            if p.requires_grad:
                numels.append(p.numel())
                shapes.append(list(p.shape) + [-1] * (4 - p.dim()))
                owner.append(i)
        mg.check(len(ema.m_name2s_name) == sum(1 for o in owner if o == i), "one shadow per trainable tensor")
        print(f"  {name}: {sum(1 for o in owner if o == i)} trainable tensors, {sum(n for n, o in zip(numels, owner) if o == i)} elements")
    out["model/parts"] = np.array([name for name, _ in parts])
    out["model/numel"] = np.array(numels, np.int64)
    out["model/shape"] = np.array(shapes, np.int32)            # [tensors, 4], -1 beyond the tensor's rank
    out["model/owner"] = np.array(owner, np.int8)
    print(f"  {len(numels)} tensors, {sum(numels)} elements, {sum(1 for n in numels if n <= 512)} of at most 512, median {int(np.median(numels))}")


def main():
    out = {}
    print("LitEma on the small module (ema.py:25-44)")
    run(out, "plain", False, 0)
    run(out, "counted", True, 0)
    run(out, "cross", True, START)
    print("trainable tensors of the model at the training config")
    model_shapes(out)
    np.savez_compressed(os.path.join(HERE, "ema.npz"), **out)


if __name__ == "__main__":
    main()
