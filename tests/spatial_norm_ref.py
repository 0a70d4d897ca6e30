"""What the SpatialNorm tests measure against (CGIC/modules/vqvae/decoder.py:34-53), on the CPU:

  restatement(...)   the layer written out in float64 with the closed form of the "nearest" index -- the reference of the GPU tests;
                     tests/test_spatial_norm_host.py holds it to tests/golden/spatial_norm.npz, which the real class produced;
  torch_fp32(...)    the same expression by torch's own fp32 CPU ops (F.interpolate, F.group_norm, F.conv2d): its max-abs error
                     against the float64 value is E_ref, the unit of the tests' bar;
  StandIn            a module with the reference's members and forward, for the module and install() tests.
"""
import numpy as np
import torch
import torch.nn.functional as F

BAR = 4.0          # the kernel's fp32 output may err by BAR * E_ref: both are the same chain of about six roundings in another order


def nearest(n, nq):
    """source index per destination index: dst // (n / nq) up-sampled, dst * (nq / n) sub-sampled"""
    assert n % nq == 0 or nq % n == 0
    d = torch.arange(n)
    return d // (n // nq) if n % nq == 0 else d * (nq // n)


def restatement(f, zq, gn_w, gn_b, wy, by, wb, bb, groups=32, eps=1e-6, swish=False):
    """float64 [B,C,H,W] from the exactly upcast inputs"""
    f, zq, gn_w, gn_b, wy, by, wb, bb = (t.detach().cpu().double() for t in (f, zq, gn_w, gn_b, wy, by, wb, bb))
    B, C, H, W = f.shape
    z = zq[:, :, nearest(H, zq.shape[2])][:, :, :, nearest(W, zq.shape[3])]
    x = f.reshape(B, groups, -1)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    n = ((x - mean) / torch.sqrt(var + eps)).reshape(B, C, H, W) * gn_w.reshape(1, C, 1, 1) + gn_b.reshape(1, C, 1, 1)
    y = torch.einsum("ck,bkhw->bchw", wy.reshape(C, -1), z) + by.reshape(1, C, 1, 1)
    b = torch.einsum("ck,bkhw->bchw", wb.reshape(C, -1), z) + bb.reshape(1, C, 1, 1)
    v = n * y + b
    return v * torch.sigmoid(v) if swish else v


def torch_fp32(f, zq, gn_w, gn_b, wy, by, wb, bb, groups=32, eps=1e-6, swish=False):
    """the reference's expression by torch's fp32 CPU ops, on the exactly upcast inputs"""
    f, zq, gn_w, gn_b, wy, by, wb, bb = (t.detach().cpu().float() for t in (f, zq, gn_w, gn_b, wy, by, wb, bb))
    C = f.shape[1]
    z = F.interpolate(zq, size=f.shape[-2:], mode="nearest")
    v = F.group_norm(f, groups, gn_w, gn_b, eps) * F.conv2d(z, wy.reshape(C, -1, 1, 1), by) + F.conv2d(z, wb.reshape(C, -1, 1, 1), bb)
    return v * torch.sigmoid(v) if swish else v


def e_ref(ref64, *args, **kw):
    """max-abs error of torch's fp32 evaluation against the float64 value, over the elements that are finite in it"""
    got = torch_fp32(*args, **kw).double()
    ok = torch.isfinite(ref64)
    return float((got - ref64)[ok].abs().max())


def max_err(got, ref64):
    """(max-abs error over the finite elements of the reference, NaN patterns equal)"""
    got = got.detach().cpu().double()
    ok = torch.isfinite(ref64)
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(ref64)))
    return (float((got - ref64)[ok].abs().max()) if bool(ok.any()) else 0.0), same_nan


def make_inputs(rng, B, C, H, W, hq, wq, dtype=torch.float32):
    """features (rounded to `dtype`), zq and the six parameter arrays: seeded, of the magnitudes a trained decoder has"""
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    f = (t(B, C, H, W) * 1.5 + 0.25).to(dtype)
    return dict(f=f, zq=t(B, 4, hq, wq), gn_w=1.0 + 0.2 * t(C), gn_b=0.1 * t(C), wy=0.5 * t(C, 4), by=1.0 + 0.1 * t(C), wb=0.5 * t(C, 4), bb=0.1 * t(C))


ORDER = ("f", "zq", "gn_w", "gn_b", "wy", "by", "wb", "bb")


class StandIn(torch.nn.Module):
    """the members and the forward of decoder.py:34-53, for tests of the module swap (not the package's class)"""

    def __init__(self, f_channels, zq_channels=4, add_conv=False, groups=32):
        super().__init__()
        self.norm_layer = torch.nn.GroupNorm(num_groups=groups, num_channels=f_channels, eps=1e-6, affine=True)
        self.add_conv = add_conv
        if add_conv:
            self.conv = torch.nn.Conv2d(zq_channels, zq_channels, kernel_size=3, stride=1, padding=1)
        self.conv_y = torch.nn.Conv2d(zq_channels, f_channels, kernel_size=1)
        self.conv_b = torch.nn.Conv2d(zq_channels, f_channels, kernel_size=1)

    def forward(self, f, zq):
        zq = F.interpolate(zq, size=f.shape[-2:], mode="nearest")
        if self.add_conv:
            zq = self.conv(zq)
        return self.norm_layer(f) * self.conv_y(zq) + self.conv_b(zq)


def randomize(module, seed):
    """parameters away from their initial values (GroupNorm starts at weight 1, bias 0), seeded"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p + 0.3 * torch.randn(p.shape, generator=g).to(p))
    return module
