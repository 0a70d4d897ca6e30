"""What the GroupNorm and ResnetBlock tests measure against (CGIC/modules/vqvae/vqvae_blocks.py:34, :29-31), on the CPU:

  restatement(...)   GroupNorm(groups, eps, affine) (+ swish) written out in float64 -- the reference of the GPU tests;
                     tests/test_group_norm_host.py holds it to torch's own float64 F.group_norm, tests/test_resblock_host.py to the
                     real ResnetBlocks' fixture through resblock64();
  torch_fp32(...)    the same by torch's own fp32 CPU F.group_norm (+ x * sigmoid(x)): its max-abs error against the float64 value
                     is E_ref, the unit of the tests' bar (spatial_norm_ref.BAR * E_ref);
  reference_grads()  per gradient tensor (f, gn_w, gn_b): the float64 autograd gradient and E_ref of the fp32 CPU autograd;
  resblock64(...)    the ResnetBlock of either kind from a state_dict, in float64, norms by the restatements.
"""
import numpy as np
import torch
import torch.nn.functional as F

import spatial_norm_ref as sref

BAR = sref.BAR
ORDER = ("f", "gn_w", "gn_b")
GRADS = ORDER


def layer64(f, gn_w, gn_b, groups=32, eps=1e-6, swish=False):
    """float64 [B,C,H,W] from float64 tensors; differentiable"""
    B, C, H, W = f.shape
    x = f.reshape(B, groups, -1)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    v = ((x - mean) / torch.sqrt(var + eps)).reshape(B, C, H, W) * gn_w.reshape(1, C, 1, 1) + gn_b.reshape(1, C, 1, 1)
    return v * torch.sigmoid(v) if swish else v


def layer32(f, gn_w, gn_b, groups=32, eps=1e-6, swish=False):
    """torch's fp32 CPU ops; differentiable"""
    v = F.group_norm(f, groups, gn_w, gn_b, eps)
    return v * torch.sigmoid(v) if swish else v


def restatement(f, gn_w, gn_b, groups=32, eps=1e-6, swish=False):
    """float64 [B,C,H,W] from the exactly upcast inputs"""
    return layer64(*(t.detach().cpu().double() for t in (f, gn_w, gn_b)), groups=groups, eps=eps, swish=swish)


def torch_fp32(f, gn_w, gn_b, groups=32, eps=1e-6, swish=False):
    return layer32(*(t.detach().cpu().float() for t in (f, gn_w, gn_b)), groups=groups, eps=eps, swish=swish)


def e_ref(ref64, *args, **kw):
    """max-abs error of torch's fp32 evaluation against the float64 value, over the elements that are finite in it"""
    got = torch_fp32(*args, **kw).double()
    ok = torch.isfinite(ref64)
    return float((got - ref64)[ok].abs().max())


max_err = sref.max_err


def make_inputs(rng, B, C, H, W, dtype=torch.float32):
    """features (rounded to `dtype`) and the two parameter arrays: seeded, of the magnitudes a trained encoder has"""
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return dict(f=(t(B, C, H, W) * 1.5 + 0.25).to(dtype), gn_w=1.0 + 0.2 * t(C), gn_b=0.1 * t(C))


def make_zq(rng, B, H, W):
    """a finite random zq at ratio 1: with conv_y = 1 and conv_b = 0 on it, spatial_norm is group_norm"""
    return torch.from_numpy(rng.standard_normal((B, 4, H, W)).astype(np.float32))


def _grads(layer, dtype, x, go, swish):
    leaves = [x[k].detach().cpu().to(dtype).requires_grad_() for k in ORDER]
    got = torch.autograd.grad(layer(*leaves, swish=swish), leaves, go.detach().cpu().to(dtype))
    return {k: g.reshape(x[k].shape) for k, g in zip(GRADS, got)}


def reference_grads(x, go, swish=False):
    """-> ({name: float64 gradient}, {name: E_ref}) of sum(out * go)"""
    g64, g32 = _grads(layer64, torch.float64, x, go, swish), _grads(layer32, torch.float32, x, go, swish)
    eref = {}
    for k in GRADS:
        ok = torch.isfinite(g64[k])
        eref[k] = float((g32[k].double() - g64[k])[ok].abs().max()) if bool(ok.any()) else 0.0
    return g64, eref


def resblock64(sd, x, zq=None):
    """the reference's ResnetBlock.forward(x, None[, zq]) in float64 from its state_dict (float64 tensors): the norms by
    restatement() / spatial_norm_ref.restatement() (with add_conv: interpolate + the 3x3 conv in front, then ratio 1)"""
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()

    def norm(prefix, h):
        if prefix + ".weight" in sd:
            return restatement(h, sd[prefix + ".weight"], sd[prefix + ".bias"])
        z = zq.double()
        if prefix + ".conv.weight" in sd:
            z = F.conv2d(F.interpolate(z, size=h.shape[-2:], mode="nearest"), sd[prefix + ".conv.weight"], sd[prefix + ".conv.bias"], padding=1)
        return sref.restatement(h, z, sd[prefix + ".norm_layer.weight"], sd[prefix + ".norm_layer.bias"], sd[prefix + ".conv_y.weight"],
                                sd[prefix + ".conv_y.bias"], sd[prefix + ".conv_b.weight"], sd[prefix + ".conv_b.bias"])

    h = norm("norm1", x)
    h = F.conv2d(h * torch.sigmoid(h), sd["conv1.weight"], sd["conv1.bias"], padding=1)
    h = norm("norm2", h)
    h = F.conv2d(h * torch.sigmoid(h), sd["conv2.weight"], sd["conv2.bias"], padding=1)
    if "conv_shortcut.weight" in sd:
        x = F.conv2d(x, sd["conv_shortcut.weight"], sd["conv_shortcut.bias"], padding=1)
    elif "nin_shortcut.weight" in sd:
        x = F.conv2d(x, sd["nin_shortcut.weight"], sd["nin_shortcut.bias"])
    return x + h


class StandInBlock(torch.nn.Module):
    """the members and the forward of the reference's ResnetBlock (vqvae_blocks.py:78-137; dec=True: decoder.py:99-158 on
    spatial_norm_ref.StandIn norms), for tests of the module swap (not the package's class)"""

    def __init__(self, cin, cout, dec=False, temb_channels=0, dropout=0.0):
        super().__init__()
        self.in_channels, self.out_channels, self.use_conv_shortcut = cin, cout, False
        mk = (lambda c: sref.StandIn(c)) if dec else (lambda c: torch.nn.GroupNorm(32, c, eps=1e-6))
        self.norm1 = mk(cin)
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, padding=1)
        if temb_channels > 0:
            self.temb_proj = torch.nn.Linear(temb_channels, cout)
        self.norm2 = mk(cout)
        self.dropout = torch.nn.Dropout(dropout)
        self.conv2 = torch.nn.Conv2d(cout, cout, 3, padding=1)
        if cin != cout:
            self.nin_shortcut = torch.nn.Conv2d(cin, cout, 1)
        self.dec = dec

    def forward(self, x, temb, zq=None):
        sw = lambda t: t * torch.sigmoid(t)
        h = self.conv1(sw(self.norm1(x, zq) if self.dec else self.norm1(x)))
        if temb is not None:
            h = h + self.temb_proj(sw(temb))[:, :, None, None]
        h = self.conv2(self.dropout(sw(self.norm2(h, zq) if self.dec else self.norm2(h))))
        return (self.nin_shortcut(x) if self.in_channels != self.out_channels else x) + h


class StandInEncoder(torch.nn.Module):
    """the reference Encoder's `down` path and head as small as they get (vqvae_blocks.py:195-351 at ch 32, ch_mult (1, 2), one
    block per level, resolution 16): conv_in, down[0] = block 32 -> 32 + strided-conv downsample, down[1] = block 32 -> 64, mid
    block 64 -> 64, norm_out + swish + conv_out -- seven GroupNorms, three ResnetBlock-shaped modules"""

    def __init__(self):
        super().__init__()
        self.conv_in = torch.nn.Conv2d(3, 32, 3, padding=1)
        self.down = torch.nn.ModuleList()
        for cin, cout, last in ((32, 32, False), (32, 64, True)):
            level = torch.nn.Module()
            level.block = torch.nn.ModuleList([StandInBlock(cin, cout)])
            if not last:
                level.downsample = torch.nn.Conv2d(cout, cout, 3, stride=2, padding=0)
            self.down.append(level)
        self.mid = torch.nn.Module()
        self.mid.block_1 = StandInBlock(64, 64)
        self.norm_out = torch.nn.GroupNorm(32, 64, eps=1e-6)
        self.conv_out = torch.nn.Conv2d(64, 4, 3, padding=1)

    def forward(self, x):
        h = self.conv_in(x)
        for level in self.down:
            for block in level.block:
                h = block(h, None)
            if hasattr(level, "downsample"):
                h = level.downsample(F.pad(h, (0, 1, 0, 1), mode="constant", value=0))
        h = self.mid.block_1(h, None)
        h = self.norm_out(h)
        return self.conv_out(h * torch.sigmoid(h))
