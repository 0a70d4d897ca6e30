"""The decoder's SpatialNorm (CGIC/modules/vqvae/decoder.py:34-53) on the library's kernel (csrc/cgic_norm.hip):

    zq    = interpolate(zq, size=f.shape[-2:], mode="nearest")
    new_f = GroupNorm(32, eps=1e-6, affine)(f) * conv_y(zq) + conv_b(zq)            # conv_y, conv_b: 1x1, 4 -> C

as one pass over the features instead of torch's six, with the swish that ResnetBlock puts behind it on request.
`spatial_norm` is the raw call with its checks (no autograd) and the one function that reaches cgic_spatial_norm;
torch.ops.cgic.spatial_norm wraps it (spatial_norm_op below: schema and fake kernel); `SpatialNorm` is the module with the reference's constructor
and state_dict keys, which model.install(..., patch_norms=True) puts in the place of the reference's.

Feature types.  fp32 features give fp32.  fp16 / bf16 features (the conv nets under torch.autocast) are read as they are -- no cast
pass -- and give fp32 as well, which is what the reference's expression returns under autocast (group_norm is on autocast's fp32
list and the products promote); `out_dtype` (or the dtype of `out`) set to the features' half type is the opt-in: the same fp32
value rounded once to nearest-even.  The kernel's conv_y / conv_b values stay in fp32 where autocast would round them to the half
type first: it is the more exact of the two.
"""
import torch

from . import _lib

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}          # CGIC_DT_* (include/cgic_hip.h)
ZQ_CHANNELS = 4


def integer_ratio(n, nq):
    """an axis of n feature rows over nq rows of zq is one the kernel indexes: up-sampled (n % nq == 0) or sub-sampled (nq % n == 0)"""
    return n > 0 and nq > 0 and (n % nq == 0 or nq % n == 0)


def nearest_index(n, nq):
    """the source index of torch's "nearest" at an integer ratio, as the kernel computes it: dst // (n / nq) up, dst * (nq / n) down"""
    if not integer_ratio(n, nq):
        raise ValueError(f"spatial_norm: {nq} rows of zq under {n} of the features is not an integer ratio")
    return [d // (n // nq) for d in range(n)] if n % nq == 0 else [d * (nq // n) for d in range(n)]


def _result_type(f, out, out_dtype):
    """the dtype of the result: fp32, or the features' half type when `out_dtype` / the dtype of `out` says so"""
    half = f.dtype if f.dtype in (torch.float16, torch.bfloat16) else None
    if out is not None:
        if out.dtype != torch.float32 and out.dtype != half:
            raise TypeError(f"spatial_norm: out is {out.dtype}; the result of these features is torch.float32" if half is None else
                            f"spatial_norm: out is {out.dtype}; expected torch.float32 or the features' {half}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError(f"spatial_norm: out_dtype {out_dtype}, but out is {out.dtype}")
        return out.dtype
    if out_dtype is None or out_dtype == torch.float32:
        return torch.float32
    if out_dtype != half:
        raise TypeError(f"spatial_norm: out_dtype {out_dtype}; expected torch.float32" + ("" if half is None else f" or the features' {half}"))
    return half


def spatial_norm(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups=32, eps=1e-6, swish=False, out=None, out_dtype=None):
    """GroupNorm(groups, eps)(f) * conv_y(zq') + conv_b(zq'), zq' = zq at f's size by "nearest"; with swish, x * sigmoid(x) of that.
    f [B,C,H,W] fp32 / fp16 / bf16; zq [B,4,hq,wq] (a half zq is cast to fp32), each axis at an integer ratio of f's, up or down;
    gn_weight, gn_bias, by, bb [C]; wy, wb the 1x1 conv weights, [C,4] or [C,4,1,1].  -> `out` (which may be `f` when the types are
    equal: in place) or a new tensor; fp32 unless out / out_dtype is the features' half type.  No autograd."""
    params = (gn_weight, gn_bias, wy, by, wb, bb)
    _lib.require_device(f, zq, *params, out)
    if f.dim() != 4 or f.dtype not in _DT:
        raise TypeError(f"spatial_norm: features {f.dtype} {tuple(f.shape)}; expected fp32, fp16 or bf16 [B,C,H,W]")
    B, C, H, W = f.shape
    groups = int(groups)
    if groups <= 0 or C % groups:
        raise ValueError(f"spatial_norm: {C} channels in {groups} groups")
    if zq.dim() != 4 or zq.shape[0] != B or zq.shape[1] != ZQ_CHANNELS or not zq.dtype.is_floating_point:
        raise ValueError(f"spatial_norm: zq {zq.dtype} {tuple(zq.shape)}; expected [{B},{ZQ_CHANNELS},hq,wq]")
    hq, wq = zq.shape[2], zq.shape[3]
    if not (integer_ratio(H, hq) and integer_ratio(W, wq)):
        raise ValueError(f"spatial_norm: zq {hq}x{wq} under features {H}x{W}: each axis must be an integer ratio, up or down")
    for name, p, n in (("gn_weight", gn_weight, C), ("gn_bias", gn_bias, C), ("wy", wy, C * ZQ_CHANNELS), ("by", by, C),
                       ("wb", wb, C * ZQ_CHANNELS), ("bb", bb, C)):
        if p.numel() != n or not p.dtype.is_floating_point or (n != C and p.shape[0] != C):
            raise ValueError(f"spatial_norm: {name} {p.dtype} {tuple(p.shape)}; expected {n} floating-point values" + ("" if n == C else f" as [{C},{ZQ_CHANNELS}]"))
    if out is not None:
        if out.device != f.device:
            raise ValueError(f"spatial_norm: out is on {out.device}, f on {f.device}")
        if tuple(out.shape) != tuple(f.shape):
            raise ValueError(f"spatial_norm: out {tuple(out.shape)} must have f's shape {tuple(f.shape)}")
        if not out.is_contiguous():
            raise ValueError("spatial_norm: out must be contiguous")
    res = _result_type(f, out, out_dtype)
    f = f.contiguous()
    zq = zq.contiguous().float()
    gn_weight, gn_bias, wy, by, wb, bb = (p.detach().contiguous().float() for p in params)
    if out is None:
        out = torch.empty_like(f, dtype=res)
    nbytes = _lib.lib().cgic_spatial_norm_workspace_bytes(_DT[f.dtype], B, C, H, W, groups)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device) if nbytes else None
    with _lib.on_device(f.device):
        _lib.call("cgic_spatial_norm", _lib.ptr(f), _DT[f.dtype], B, C, H, W, _lib.ptr(zq), hq, wq, groups, float(eps), _lib.ptr(gn_weight),
                  _lib.ptr(gn_bias), _lib.ptr(wy), _lib.ptr(by), _lib.ptr(wb), _lib.ptr(bb), int(bool(swish)), _lib.ptr(out), _DT[res],
                  _lib.ptr(ws), nbytes, _lib.current_stream(f.device))
    return out


@torch.library.custom_op("cgic::spatial_norm", mutates_args=(), device_types="cuda")
def spatial_norm_op(f: torch.Tensor, zq: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, wy: torch.Tensor, by: torch.Tensor,
                    wb: torch.Tensor, bb: torch.Tensor, groups: int, eps: float, swish: bool, half_out: bool) -> torch.Tensor:
    """torch.ops.cgic.spatial_norm: spatial_norm as a custom op (schema, fake kernel; inference only -- no autograd formula, the
    module takes torch's own expression when a gradient is needed): fp32 [B,C,H,W], or with half_out the type of f"""
    return spatial_norm(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups=groups, eps=eps, swish=swish, out_dtype=f.dtype if half_out else None)


@spatial_norm_op.register_fake
def _(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups, eps, swish, half_out):
    return f.new_empty(f.shape, dtype=f.dtype if half_out else torch.float32)


def one_launch(dtype, B, C, H, W, groups=32):
    """the form the library's plan picks for features of this type and shape: True one launch (one workgroup per group), False
    two (statistics, then apply).  cgic_spatial_norm_one_launch: tests take their shapes either side of the boundary from here"""
    return bool(_lib.call("cgic_spatial_norm_one_launch", _DT[dtype], B, C, H, W, int(groups)))


def has_reference_shape(m):
    """`m` has the members of the reference's SpatialNorm (decoder.py:34-53): norm_layer, 1x1 conv_y / conv_b from one zq, add_conv"""
    cy, cb = getattr(m, "conv_y", None), getattr(m, "conv_b", None)
    return (isinstance(getattr(m, "norm_layer", None), torch.nn.Module) and hasattr(m, "add_conv")
            and all(isinstance(c, torch.nn.Conv2d) and c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) and c.groups == 1
                    for c in (cy, cb))
            and cy.in_channels == cb.in_channels and cy.out_channels == cb.out_channels
            and (not m.add_conv or isinstance(getattr(m, "conv", None), torch.nn.Conv2d)))


class SpatialNorm(torch.nn.Module):
    """decoder.py:34-53 with the reference's constructor and state_dict keys (norm_layer.weight / bias, conv_y.*, conv_b.*, conv.*).
    forward(f, zq) is the reference's; forward(f, zq, swish=True) also applies the swish that ResnetBlock puts behind it
    (decoder.py:141,148).  The kernel serves the call when the tensors are on the device, no autograd is needed, the norm layer is
    an affine GroupNorm, zq has 4 channels and both axes are at integer ratios; anything else evaluates the reference's expression
    with torch ops."""

    def __init__(self, f_channels, zq_channels, norm_layer=torch.nn.GroupNorm, freeze_norm_layer=False, add_conv=False, **norm_layer_params):
        super().__init__()
        self.norm_layer = norm_layer(num_channels=f_channels, **norm_layer_params)
        if freeze_norm_layer:
            for p in self.norm_layer.parameters():
                p.requires_grad = False
        self.add_conv = add_conv
        if self.add_conv:
            self.conv = torch.nn.Conv2d(zq_channels, zq_channels, kernel_size=3, stride=1, padding=1)
        self.conv_y = torch.nn.Conv2d(zq_channels, f_channels, kernel_size=1, stride=1, padding=0)
        self.conv_b = torch.nn.Conv2d(zq_channels, f_channels, kernel_size=1, stride=1, padding=0)

    @classmethod
    def adopt(cls, module):
        """a SpatialNorm on the SAME submodules as `module` (a reference SpatialNorm): the parameter objects and the state_dict
        keys stay what they are"""
        if not has_reference_shape(module):
            raise TypeError(f"SpatialNorm.adopt: {type(module).__name__} has not the reference's norm_layer / 1x1 conv_y / conv_b / add_conv")
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.norm_layer = module.norm_layer
        m.add_conv = module.add_conv
        if m.add_conv:
            m.conv = module.conv
        m.conv_y, m.conv_b = module.conv_y, module.conv_b
        m.train(module.training)
        return m

    def uses_kernel(self, f, zq):
        """the kernel serves this call (otherwise: the reference's expression in torch ops)"""
        gn = self.norm_layer
        if not (f.is_cuda and zq.is_cuda and f.dim() == 4 and zq.dim() == 4 and f.dtype in _DT and zq.dtype in _DT):
            return False
        if not (isinstance(gn, torch.nn.GroupNorm) and gn.affine and gn.num_channels == f.shape[1] and self.conv_y.out_channels == f.shape[1]):
            return False
        if zq.shape[1] != ZQ_CHANNELS or self.conv_y.in_channels != ZQ_CHANNELS or zq.shape[0] != f.shape[0]:
            return False
        if self.conv_y.bias is None or self.conv_b.bias is None:
            return False
        if torch.is_grad_enabled() and (f.requires_grad or zq.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return self.add_conv or (integer_ratio(f.shape[2], zq.shape[2]) and integer_ratio(f.shape[3], zq.shape[3]))

    def forward(self, f, zq, swish=False, out_dtype=None):
        if self.uses_kernel(f, zq):
            if self.add_conv:                   # the 3x3 conv works on the interpolated zq: both stay torch's, the kernel runs at ratio 1
                zq = self.conv(torch.nn.functional.interpolate(zq, size=f.shape[-2:], mode="nearest"))
            gn = self.norm_layer
            half = out_dtype is not None and out_dtype != torch.float32
            if half and out_dtype != f.dtype:
                raise TypeError(f"SpatialNorm: out_dtype {out_dtype}; expected torch.float32 or the features' {f.dtype}")
            return torch.ops.cgic.spatial_norm(f, zq, gn.weight, gn.bias, self.conv_y.weight, self.conv_y.bias, self.conv_b.weight,
                                               self.conv_b.bias, gn.num_groups, gn.eps, bool(swish), half)
        zq = torch.nn.functional.interpolate(zq, size=f.shape[-2:], mode="nearest")
        if self.add_conv:
            zq = self.conv(zq)
        new_f = self.norm_layer(f) * self.conv_y(zq) + self.conv_b(zq)
        if swish:
            new_f = new_f * torch.sigmoid(new_f)
        return new_f if out_dtype is None else new_f.to(out_dtype)


def patch_norms(model):
    """swap every module of `model` that has the reference SpatialNorm's shape for norm.SpatialNorm on the same submodules;
    -> the number swapped"""
    found = [(parent, name) for parent in model.modules() for name, child in parent.named_children()
             if not isinstance(child, SpatialNorm) and has_reference_shape(child)]
    for parent, name in found:
        setattr(parent, name, SpatialNorm.adopt(getattr(parent, name)))
    return len(found)
