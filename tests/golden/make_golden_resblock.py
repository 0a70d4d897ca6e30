"""Writes tests/golden/resblock.npz from the REAL ResnetBlocks (CGIC/modules/vqvae/vqvae_blocks.py:78-137 the encoder's,
decoder.py:99-158 the decoder's), run on the CPU in float64 and in float32.  Data only: per case the inputs, the state_dict, the
float64 result, the reference's own fp32 max-abs error against it, and the state_dict keys.  While it writes, it holds
tests/group_norm_ref.py's float64 restatement of the block to the class.

    python tests/golden/make_golden_resblock.py <root of the reference checkout>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import group_norm_ref as gref       # noqa: E402
import spatial_norm_ref as sref     # noqa: E402

# name: kind, B, in, out, H, W, conv_shortcut, (hq, wq) or None, add_conv
CASES = {
    "enc_same": ("enc", 1, 32, 32, 4, 6, False, None, False),
    "enc_nin": ("enc", 1, 32, 64, 6, 10, False, None, False),
    "enc_conv_shortcut": ("enc", 1, 32, 64, 4, 6, True, None, False),
    "dec_zq": ("dec", 1, 32, 64, 4, 6, False, (2, 3), False),
    "dec_add_conv": ("dec", 1, 32, 64, 4, 6, False, (2, 3), True),
}


def sparse_convs(module, seed):
    """the 3x3 and shortcut conv weights as sparse ternary values (one tap in 32, +-1/4): real convolutions of the same
    magnitude whose 265 000 weights deflate to a few KB, so the fixture stays small; every other parameter stays randomize()'s"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in module.named_parameters():
            if p.dim() == 4 and k.split(".")[0] in ("conv1", "conv2", "conv_shortcut", "nin_shortcut"):
                keep = torch.rand(p.shape, generator=g) < 1.0 / 32
                sign = torch.where(torch.rand(p.shape, generator=g) < 0.5, -0.25, 0.25)
                p.copy_(torch.where(keep, sign, torch.zeros(())).to(p))
    return module


def main(reference_root):
    sys.path.insert(0, reference_root)
    from CGIC.modules.vqvae import decoder, vqvae_blocks
    out = {}
    for i, (name, (kind, B, cin, cout, H, W, conv_shortcut, zq_grid, add_conv)) in enumerate(CASES.items()):
        torch.manual_seed(400 + i)
        if kind == "enc":
            m = vqvae_blocks.ResnetBlock(in_channels=cin, out_channels=cout, conv_shortcut=conv_shortcut, dropout=0.0, temb_channels=0)
        else:
            m = decoder.ResnetBlock(in_channels=cin, out_channels=cout, conv_shortcut=conv_shortcut, dropout=0.0, temb_channels=0, zq_ch=4,
                                    add_conv=add_conv)
        m = sparse_convs(sref.randomize(m, 500 + i), 550 + i).eval()
        rng = np.random.default_rng(600 + i)
        x = torch.from_numpy(rng.standard_normal((B, cin, H, W)).astype(np.float32)) * 1.5 + 0.25
        zq = None if zq_grid is None else torch.from_numpy(rng.standard_normal((B, 4, *zq_grid)).astype(np.float32))
        args32 = (x, None) if zq is None else (x, None, zq)
        args64 = (x.double(), None) if zq is None else (x.double(), None, zq.double())
        with torch.no_grad():
            got32 = m(*args32).double()
            m64 = m.double()
            got64 = m64(*args64)
        sd = m64.state_dict()
        mine = gref.resblock64(sd, x, zq)
        assert float((mine - got64).abs().max()) < 1e-12, name
        out[name + "/shape"] = np.array([B, cin, cout, H, W, int(conv_shortcut), int(add_conv), int(kind == "dec")], np.int64)
        out[name + "/x"] = x.numpy()
        if zq is not None:
            out[name + "/zq"] = zq.numpy()
        for k, v in sd.items():
            out[name + "/sd/" + k] = v.float().numpy()          # (randomize() made them from fp32 values: exact)
        out[name + "/ref64"] = got64.numpy()
        out[name + "/err32"] = np.array(float((got32 - got64).abs().max()))
        out[name + "/keys"] = np.array(list(sd.keys()))
    np.savez_compressed(os.path.join(HERE, "resblock.npz"), **out)
    print({k.split("/")[0]: float(v) for k, v in out.items() if k.endswith("/err32")})


if __name__ == "__main__":
    main(sys.argv[1])
