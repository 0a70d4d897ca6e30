"""Writes tests/golden/spatial_norm.npz from the REAL SpatialNorm (CGIC/modules/vqvae/decoder.py:34-53), run on the CPU in float64
and in float32.  Data only: per case the inputs and parameters, the float64 result, and the reference's own fp32 max-abs error
against it; and the class's state_dict keys.  While it writes, it holds tests/spatial_norm_ref.py's float64 restatement (the
closed-form "nearest" index included) to the class.

    python tests/golden/make_golden_norm.py <root of the reference checkout>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import spatial_norm_ref as ref      # noqa: E402

# name: B, C, H, W, hq, wq, add_conv -- up-sampled, equal, sub-sampled, the axes at different ratios
CASES = {
    "up2": (2, 32, 4, 6, 2, 3, False),
    "up4_up2": (1, 64, 8, 12, 2, 6, False),
    "same": (2, 32, 6, 10, 6, 10, False),
    "down4": (1, 32, 6, 10, 24, 40, False),
    "down4_up2": (1, 64, 2, 8, 8, 4, False),
    "add_conv": (1, 32, 4, 4, 2, 2, True),
}


def main(reference_root):
    sys.path.insert(0, reference_root)
    from CGIC.modules.vqvae.decoder import SpatialNorm
    out = {}
    for i, (name, (B, C, H, W, hq, wq, add_conv)) in enumerate(CASES.items()):
        torch.manual_seed(100 + i)
        m = ref.randomize(SpatialNorm(C, 4, add_conv=add_conv, num_groups=32, eps=1e-6, affine=True), 200 + i).eval()
        x = ref.make_inputs(np.random.default_rng(300 + i), B, C, H, W, hq, wq)
        with torch.no_grad():
            got32 = m(x["f"], x["zq"]).double()
            m64 = m.double()
            got64 = m64(x["f"].double(), x["zq"].double())
        sd = m64.state_dict()
        if not add_conv:
            mine = ref.restatement(x["f"], x["zq"], sd["norm_layer.weight"], sd["norm_layer.bias"], sd["conv_y.weight"], sd["conv_y.bias"],
                                   sd["conv_b.weight"], sd["conv_b.bias"])
            assert float((mine - got64).abs().max()) < 1e-12, name
        out[name + "/shape"] = np.array([B, C, H, W, hq, wq, int(add_conv)], np.int64)
        out[name + "/f"] = x["f"].numpy()
        out[name + "/zq"] = x["zq"].numpy()
        for k, v in sd.items():
            out[name + "/" + k] = v.float().numpy()         # (randomize() made them from fp32 values: exact)
        out[name + "/ref64"] = got64.numpy()
        out[name + "/err32"] = np.array(float((got32 - got64).abs().max()))
        out[name + "/keys"] = np.array(list(sd.keys()))
    np.savez_compressed(os.path.join(HERE, "spatial_norm.npz"), **out)
    print({k.split("/")[0]: float(v) for k, v in out.items() if k.endswith("/err32")})


if __name__ == "__main__":
    main(sys.argv[1])
