"""The reference's ResnetBlock (CGIC/modules/vqvae/vqvae_blocks.py:78-137 the encoder's, decoder.py:99-158 the decoder's) with the
swish fused into the normalisation in front of each conv:

    h = conv1(swish(norm1(x)));  h = conv2(dropout(swish(norm2(h))));  return shortcut(x) + h

In the reference the swish is inline in forward(), so the `swish=1` of the library's norm kernels (csrc/cgic_norm.hip) cannot be
reached by swapping the norms alone.  `ResnetBlock` has both reference constructors, the reference's state_dict keys (norm1.*,
conv1.*, temb_proj.*, norm2.*, conv2.*, conv_shortcut.* / nin_shortcut.*) and an adopt(); model.install(..., patch_resblocks=True)
puts it in the place of the reference's.  Where norm1 / norm2 are the library's modules (norm.GroupNorm, norm.SpatialNorm) the swish
rides in the norm call; any other norm is called as the reference calls it and followed by x * sigmoid(x).  The convs, the dropout
and the residual add are torch's either way.

Under torch.autocast the reference's norm and swish give fp32 (group_norm is on autocast's fp32 list) and autocast casts that to the
half type in front of the conv.  When the features already are of the autocast type, the dropout does nothing (p == 0 or eval) and
the norm takes a kernel route, the block asks the kernel for the half type directly: the fp32 swish rounded once, which is what that
cast would have produced, without the fp32 tensor in between.  With an active dropout both norms keep fp32, as in the reference.
"""
import torch

from . import norm as _norm


def has_reference_shape(m):
    """`m` has the members of the reference's ResnetBlock: norm1, conv1, norm2, dropout, conv2, in_channels, out_channels,
    use_conv_shortcut -- and the shortcut conv its channel counts call for"""
    if not all(isinstance(getattr(m, k, None), torch.nn.Module) for k in ("norm1", "norm2")):
        return False
    if not all(isinstance(getattr(m, k, None), torch.nn.Conv2d) for k in ("conv1", "conv2")):
        return False
    if not isinstance(getattr(m, "dropout", None), torch.nn.Dropout):
        return False
    if not all(hasattr(m, k) for k in ("in_channels", "out_channels", "use_conv_shortcut")):
        return False
    if m.in_channels != m.out_channels:
        return isinstance(getattr(m, "conv_shortcut" if m.use_conv_shortcut else "nin_shortcut", None), torch.nn.Conv2d)
    return True


def _takes_zq(norm):
    return isinstance(norm, _norm.SpatialNorm) or _norm.has_reference_shape(norm)


class ResnetBlock(torch.nn.Module):
    """ResnetBlock(in_channels=..., out_channels=None, conv_shortcut=False, dropout=..., temb_channels=512) is the encoder's (two
    GroupNorms, forward(x, temb)); with zq_ch (and add_conv) the decoder's (two SpatialNorms, forward(x, temb, zq)).  The norms built
    here are the library's modules; adopt() keeps whatever norms the adopted block has."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout, temb_channels=512, zq_ch=None, add_conv=False):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut

        def normalize(ch):
            if zq_ch is None:
                return _norm.GroupNorm(num_groups=32, num_channels=ch, eps=1e-6, affine=True)
            return _norm.SpatialNorm(ch, zq_ch, norm_layer=torch.nn.GroupNorm, freeze_norm_layer=False, add_conv=add_conv, num_groups=32,
                                     eps=1e-6, affine=True)

        self.norm1 = normalize(in_channels)
        self.conv1 = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if temb_channels > 0:
            self.temb_proj = torch.nn.Linear(temb_channels, out_channels)
        self.norm2 = normalize(out_channels)
        self.dropout = torch.nn.Dropout(dropout)
        self.conv2 = torch.nn.Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        if self.in_channels != self.out_channels:
            if self.use_conv_shortcut:
                self.conv_shortcut = torch.nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
            else:
                self.nin_shortcut = torch.nn.Conv2d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)

    @classmethod
    def adopt(cls, module):
        """a ResnetBlock on the SAME submodules as `module` (a reference ResnetBlock of either kind): the parameter objects and the
        state_dict keys stay what they are"""
        if not has_reference_shape(module):
            raise TypeError(f"ResnetBlock.adopt: {type(module).__name__} has not the reference's norm1 / conv1 / norm2 / dropout / conv2 / shortcut")
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.in_channels, m.out_channels, m.use_conv_shortcut = module.in_channels, module.out_channels, module.use_conv_shortcut
        m.norm1, m.conv1 = module.norm1, module.conv1
        if isinstance(getattr(module, "temb_proj", None), torch.nn.Module):
            m.temb_proj = module.temb_proj
        m.norm2, m.dropout, m.conv2 = module.norm2, module.dropout, module.conv2
        for k in ("conv_shortcut", "nin_shortcut"):
            if isinstance(getattr(module, k, None), torch.nn.Module):
                setattr(m, k, getattr(module, k))
        m.train(module.training)
        return m

    def uses_kernel(self, x, zq=None):
        """both norms of this call run on the library's kernels (the inference or the training ones), swish fused"""
        if x.dim() != 4 or self._norm_route(self.norm1, x, zq) == "torch":
            return False
        # what conv1 hands to norm2: its shape, type and need of a gradient (one element of storage)
        dtype = torch.get_autocast_dtype("cuda") if x.is_cuda and torch.is_autocast_enabled("cuda") else self.conv1.weight.dtype
        h = torch.empty(1, dtype=dtype, device=x.device).expand(x.shape[0], self.out_channels, x.shape[2], x.shape[3])
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.conv1.parameters())):
            h = h.requires_grad_()
        return self._norm_route(self.norm2, h, zq) != "torch"

    @staticmethod
    def _norm_route(norm, h, zq):
        if isinstance(norm, _norm.GroupNorm):
            return norm._route(h)
        if isinstance(norm, _norm.SpatialNorm) and zq is not None:
            return norm._route(h, zq)
        return "torch"

    def _norm_swish(self, norm, h, zq, dropout_active):
        """swish(norm(h)): in one kernel call where the norm is the library's, else as the reference writes it"""
        fused = isinstance(norm, (_norm.GroupNorm, _norm.SpatialNorm))
        if fused:
            out_dtype = None
            if (h.is_cuda and torch.is_autocast_enabled("cuda") and h.dtype == torch.get_autocast_dtype("cuda") and not dropout_active
                    and self._norm_route(norm, h, zq) != "torch"):
                out_dtype = h.dtype             # the fp32 swish rounded once: autocast's own cast in front of the conv
            return norm(h, zq, swish=True, out_dtype=out_dtype) if isinstance(norm, _norm.SpatialNorm) else norm(h, swish=True, out_dtype=out_dtype)
        h = norm(h, zq) if _takes_zq(norm) else norm(h)
        return h * torch.sigmoid(h)

    def forward(self, x, temb, zq=None):
        dropout_active = self.dropout.training and self.dropout.p > 0
        h = self._norm_swish(self.norm1, x, zq, dropout_active)
        h = self.conv1(h)
        if temb is not None:
            t = self.temb_proj(temb * torch.sigmoid(temb))
            h = h + t[:, :, None, None]
        h = self._norm_swish(self.norm2, h, zq, dropout_active)
        h = self.dropout(h)
        h = self.conv2(h)
        if self.in_channels != self.out_channels:
            x = self.conv_shortcut(x) if self.use_conv_shortcut else self.nin_shortcut(x)
        return x + h


def patch_resblocks(model):
    """swap every module of `model` that has the reference ResnetBlock's shape for resblock.ResnetBlock on the same submodules;
    -> the number swapped"""
    found = [(parent, name) for parent in model.modules() for name, child in parent.named_children()
             if not isinstance(child, ResnetBlock) and has_reference_shape(child)]
    for parent, name in found:
        setattr(parent, name, ResnetBlock.adopt(getattr(parent, name)))
    return len(found)
