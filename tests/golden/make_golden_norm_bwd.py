"""Writes tests/golden/spatial_norm_bwd.npz from the REAL SpatialNorm (CGIC/modules/vqvae/decoder.py:34-53) under float64
autograd on the CPU, with and without add_conv.  Data only: per case the inputs, the parameters, the gradient of the output (go),
and the float64 gradients of f, zq and every parameter, without and with the swish that ResnetBlock puts behind the layer.
tests/test_spatial_norm_bwd_host.py holds the gradients of tests/spatial_norm_bwd_ref.py's restatement to them.

    python tests/golden/make_golden_norm_bwd.py <root of the reference checkout>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spatial_norm_ref as ref      # noqa: E402

# name: B, C, H, W, hq, wq, add_conv -- y up-sampled and x sub-sampled; add_conv (up-sampled, then the 3x3 conv)
CASES = {
    "up2_down2": (2, 32, 4, 3, 2, 6, False),
    "add_conv": (2, 32, 4, 4, 2, 2, True),
}


def main(reference_root):
    sys.path.insert(0, reference_root)
    from CGIC.modules.vqvae.decoder import SpatialNorm
    out = {}
    for i, (name, (B, C, H, W, hq, wq, add_conv)) in enumerate(CASES.items()):
        torch.manual_seed(400 + i)
        m = ref.randomize(SpatialNorm(C, 4, add_conv=add_conv, num_groups=32, eps=1e-6, affine=True), 500 + i).double()
        rng = np.random.default_rng(600 + i)
        x = ref.make_inputs(rng, B, C, H, W, hq, wq)
        go = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
        out[name + "/shape"] = np.array([B, C, H, W, hq, wq, int(add_conv)], np.int64)
        out[name + "/f"], out[name + "/zq"], out[name + "/go"] = x["f"].numpy(), x["zq"].numpy(), go.numpy()
        names = [k for k, _ in m.named_parameters()]
        out[name + "/keys"] = np.array(names)
        for k, v in m.state_dict().items():
            out[name + "/" + k] = v.float().numpy()         # (randomize() made them from fp32 values: exact)
        for swish in (False, True):
            f, zq = x["f"].double().requires_grad_(), x["zq"].double().requires_grad_()
            v = m(f, zq)
            if swish:
                v = v * torch.sigmoid(v)
            grads = torch.autograd.grad(v, [f, zq] + [p for _, p in m.named_parameters()], go.double())
            for k, g in zip(["f", "zq"] + names, grads):
                out[f"{name}/grad{int(swish)}/{k}"] = g.numpy()
    np.savez_compressed(os.path.join(HERE, "spatial_norm_bwd.npz"), **out)
    print({k: v.shape for k, v in out.items() if "/grad1/" in k})


if __name__ == "__main__":
    main(sys.argv[1])
