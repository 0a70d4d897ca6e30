"""What the SpatialNorm backward tests measure against, on the CPU (spatial_norm_ref.restatement detaches its inputs, so it cannot
be differentiated):

  layer64(...)     the layer written out in float64 from the exactly upcast inputs, differentiable -- tests/test_spatial_norm_bwd_host.py
                   holds its gradients to tests/golden/spatial_norm_bwd.npz, which the real class gave under float64 autograd;
  layer32(...)     the same expression by torch's own fp32 CPU ops (F.interpolate, F.group_norm, F.conv2d), differentiable;
  reference(...)   per gradient tensor: the float64 gradient and E_ref, the max-abs error of the fp32 CPU gradient against it, for
                   a seeded go -- the unit of the tests' bar (spatial_norm_ref.BAR * E_ref per tensor).
"""
import numpy as np
import torch
import torch.nn.functional as F

import spatial_norm_ref as ref

GRADS = ("f", "zq", "gn_w", "gn_b", "wy", "by", "wb", "bb")           # spatial_norm_ref.ORDER: a gradient per input


def layer64(f, zq, gn_w, gn_b, wy, by, wb, bb, groups=32, eps=1e-6, swish=False):
    """float64 [B,C,H,W]; the arguments are float64 tensors (leaves that require a gradient, for autograd)"""
    B, C, H, W = f.shape
    z = zq[:, :, ref.nearest(H, zq.shape[2])][:, :, :, ref.nearest(W, zq.shape[3])]
    x = f.reshape(B, groups, -1)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    n = ((x - mean) / torch.sqrt(var + eps)).reshape(B, C, H, W) * gn_w.reshape(1, C, 1, 1) + gn_b.reshape(1, C, 1, 1)
    y = torch.einsum("ck,bkhw->bchw", wy.reshape(C, -1), z) + by.reshape(1, C, 1, 1)
    b = torch.einsum("ck,bkhw->bchw", wb.reshape(C, -1), z) + bb.reshape(1, C, 1, 1)
    v = n * y + b
    return v * torch.sigmoid(v) if swish else v


def layer32(f, zq, gn_w, gn_b, wy, by, wb, bb, groups=32, eps=1e-6, swish=False):
    """the reference's expression by torch's fp32 CPU ops"""
    C = f.shape[1]
    z = F.interpolate(zq, size=f.shape[-2:], mode="nearest")
    v = F.group_norm(f, groups, gn_w, gn_b, eps) * F.conv2d(z, wy.reshape(C, -1, 1, 1), by) + F.conv2d(z, wb.reshape(C, -1, 1, 1), bb)
    return v * torch.sigmoid(v) if swish else v


def _grads(layer, dtype, x, go, swish):
    leaves = [x[k].detach().cpu().to(dtype).requires_grad_() for k in ref.ORDER]
    out = layer(*leaves, swish=swish)
    got = torch.autograd.grad(out, leaves, go.detach().cpu().to(dtype))
    return {k: g.reshape(x[k].shape) for k, g in zip(GRADS, got)}


def grads64(x, go, swish=False):
    """{name: float64 gradient} of sum(out * go) from the exactly upcast inputs"""
    return _grads(layer64, torch.float64, x, go, swish)


def grads32(x, go, swish=False):
    """the same by torch's fp32 CPU ops and their own backward passes"""
    return _grads(layer32, torch.float32, x, go, swish)


def make_go(rng, shape, dtype=torch.float32):
    """a seeded gradient of the output, rounded to `dtype` (so that a half and a fp32 go of one test hold the same values)"""
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype)


def reference(x, go, swish=False):
    """-> ({name: float64 gradient}, {name: E_ref})"""
    g64, g32 = grads64(x, go, swish), grads32(x, go, swish)
    eref = {}
    for k in GRADS:
        ok = torch.isfinite(g64[k])
        eref[k] = float((g32[k].double() - g64[k])[ok].abs().max()) if bool(ok.any()) else 0.0
    return g64, eref
