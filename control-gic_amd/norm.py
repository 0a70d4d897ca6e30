"""The decoder's SpatialNorm (CGIC/modules/vqvae/decoder.py:34-53) on the library's kernels (csrc/cgic_norm.hip, the backward: csrc/cgic_norm_bwd.hip):

    zq    = interpolate(zq, size=f.shape[-2:], mode="nearest")
    new_f = GroupNorm(32, eps=1e-6, affine)(f) * conv_y(zq) + conv_b(zq)            # conv_y, conv_b: 1x1, 4 -> C

as one pass over the features instead of torch's six, with the swish that ResnetBlock puts behind it on request.
`spatial_norm` is the raw call with its checks (no autograd) and the one function that reaches cgic_spatial_norm;
torch.ops.cgic.spatial_norm wraps it (spatial_norm_op below: schema and fake kernel).  For training, `spatial_norm_train` is the
same forward that also returns the groups' (mean, rstd), `spatial_norm_backward` the gradients of everything from those (three
launches, deterministic), and torch.ops.cgic.spatial_norm_train the differentiable op on the two.  `SpatialNorm` is the module with the reference's constructor
and state_dict keys, which model.install(..., patch_norms=True) puts in the place of the reference's.

The encoder's plain GroupNorm (vqvae_blocks.py:34: GroupNorm(32, eps=1e-6, affine), with the swish of ResnetBlock and the norm_out
heads on request) runs on the same kernel family instantiated without zq: `group_norm`, `group_norm_train`, `group_norm_backward`,
torch.ops.cgic.group_norm / group_norm_train and the module `GroupNorm`, a torch.nn.GroupNorm subclass that
model.install(..., patch_group_norms=True) puts in the place of torch's.  The calls with and without zq share every check below.

Feature types.  fp32 features give fp32.  fp16 / bf16 features (the conv nets under torch.autocast) are read as they are -- no cast
pass -- and give fp32 as well, which is what the reference's expression returns under autocast (group_norm is on autocast's fp32
list and the products promote); `out_dtype` (or the dtype of `out`) set to the features' half type is the opt-in: the same fp32
value rounded once to nearest-even.  The kernel's conv_y / conv_b values stay in fp32 where autocast would round them to the half
type first: it is the more exact of the two.
"""
from typing import Tuple

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


def _result_type(f, out, out_dtype, name="spatial_norm"):
    """the dtype of the result: fp32, or the features' half type when `out_dtype` / the dtype of `out` says so"""
    half = f.dtype if f.dtype in (torch.float16, torch.bfloat16) else None
    if out is not None:
        if out.dtype != torch.float32 and out.dtype != half:
            raise TypeError(f"{name}: out is {out.dtype}; the result of these features is torch.float32" if half is None else
                            f"{name}: out is {out.dtype}; expected torch.float32 or the features' {half}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError(f"{name}: out_dtype {out_dtype}, but out is {out.dtype}")
        return out.dtype
    if out_dtype is None or out_dtype == torch.float32:
        return torch.float32
    if out_dtype != half:
        raise TypeError(f"{name}: out_dtype {out_dtype}; expected torch.float32" + ("" if half is None else f" or the features' {half}"))
    return half


def _check_call(name, f, zq, params, groups):
    """the checks that the forward, the training forward and the backward share, all before any data_ptr: -> B, C, H, W, hq, wq, groups.
    zq None: the plain GroupNorm, whose params are (gn_weight, gn_bias) alone; hq = wq = 0"""
    if f.dim() != 4 or f.dtype not in _DT:
        raise TypeError(f"{name}: features {f.dtype} {tuple(f.shape)}; expected fp32, fp16 or bf16 [B,C,H,W]")
    B, C, H, W = f.shape
    groups = int(groups)
    if groups <= 0 or C % groups:
        raise ValueError(f"{name}: {C} channels in {groups} groups")
    if zq is None:
        for pname, p in zip(("gn_weight", "gn_bias"), params):
            if p.numel() != C or not p.dtype.is_floating_point:
                raise ValueError(f"{name}: {pname} {p.dtype} {tuple(p.shape)}; expected {C} floating-point values")
        return B, C, H, W, 0, 0, groups
    if zq.dim() != 4 or zq.shape[0] != B or zq.shape[1] != ZQ_CHANNELS or not zq.dtype.is_floating_point:
        raise ValueError(f"{name}: zq {zq.dtype} {tuple(zq.shape)}; expected [{B},{ZQ_CHANNELS},hq,wq]")
    hq, wq = zq.shape[2], zq.shape[3]
    if not (integer_ratio(H, hq) and integer_ratio(W, wq)):
        raise ValueError(f"{name}: zq {hq}x{wq} under features {H}x{W}: each axis must be an integer ratio, up or down")
    for pname, p, n in zip(("gn_weight", "gn_bias", "wy", "by", "wb", "bb"), params, (C, C, C * ZQ_CHANNELS, C, C * ZQ_CHANNELS, C)):
        if p.numel() != n or not p.dtype.is_floating_point or (n != C and p.shape[0] != C):
            raise ValueError(f"{name}: {pname} {p.dtype} {tuple(p.shape)}; expected {n} floating-point values" + ("" if n == C else f" as [{C},{ZQ_CHANNELS}]"))
    return B, C, H, W, hq, wq, groups


def _check_out(name, f, out):
    if out is not None:
        if out.device != f.device:
            raise ValueError(f"{name}: out is on {out.device}, f on {f.device}")
        if tuple(out.shape) != tuple(f.shape):
            raise ValueError(f"{name}: out {tuple(out.shape)} must have f's shape {tuple(f.shape)}")
        if not out.is_contiguous():
            raise ValueError(f"{name}: out must be contiguous")


def _forward(name, train, f, zq, params, groups, eps, swish, out, out_dtype):
    """spatial_norm, group_norm (zq None, two parameters) and their _train forms: the checks, then the one call of cgic_<name>"""
    plain = zq is None
    _lib.require_device(f, *(() if plain else (zq,)), *params, out)
    B, C, H, W, hq, wq, groups = _check_call(name, f, zq, params, groups)
    _check_out(name, f, out)
    res = _result_type(f, out, out_dtype, name)
    f = f.contiguous()
    params = tuple(p.detach().contiguous().float() for p in params)
    if out is None:
        out = torch.empty_like(f, dtype=res)
    stats = torch.empty((B * groups, 2), dtype=torch.float32, device=f.device) if train else None
    nbytes = _lib.lib().cgic_spatial_norm_workspace_bytes(_DT[f.dtype], B, C, H, W, groups)        # (the shape's: one function for both)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=f.device) if nbytes else None
    if plain:
        mid = (groups, float(eps), *(_lib.ptr(p) for p in params))
    else:
        zq = zq.contiguous().float()
        mid = (_lib.ptr(zq), hq, wq, groups, float(eps), *(_lib.ptr(p) for p in params))
    tail = (_lib.ptr(stats),) if train else ()
    with _lib.on_device(f.device):
        _lib.call("cgic_" + name, _lib.ptr(f), _DT[f.dtype], B, C, H, W, *mid, int(bool(swish)), _lib.ptr(out), _DT[res], *tail, _lib.ptr(ws), nbytes,
                  _lib.current_stream(f.device))
    return out, stats


def spatial_norm(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups=32, eps=1e-6, swish=False, out=None, out_dtype=None):
    """GroupNorm(groups, eps)(f) * conv_y(zq') + conv_b(zq'), zq' = zq at f's size by "nearest"; with swish, x * sigmoid(x) of that.
    f [B,C,H,W] fp32 / fp16 / bf16; zq [B,4,hq,wq] (a half zq is cast to fp32), each axis at an integer ratio of f's, up or down;
    gn_weight, gn_bias, by, bb [C]; wy, wb the 1x1 conv weights, [C,4] or [C,4,1,1].  -> `out` (which may be `f` when the types are
    equal: in place) or a new tensor; fp32 unless out / out_dtype is the features' half type.  No autograd."""
    return _forward("spatial_norm", False, f, zq, (gn_weight, gn_bias, wy, by, wb, bb), groups, eps, swish, out, out_dtype)[0]


def spatial_norm_train(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups=32, eps=1e-6, swish=False, out=None, out_dtype=None):
    """spatial_norm that also returns what its backward needs besides its inputs: -> (out, stats), out bit for bit spatial_norm's,
    stats fp32 [B * groups, 2] = (mean, rstd) of each group as the kernel rounded them (cgic_spatial_norm_train).  No autograd:
    torch.ops.cgic.spatial_norm_train is the differentiable form."""
    return _forward("spatial_norm_train", True, f, zq, (gn_weight, gn_bias, wy, by, wb, bb), groups, eps, swish, out, out_dtype)


def group_norm(f, gn_weight, gn_bias, groups=32, eps=1e-6, swish=False, out=None, out_dtype=None):
    """GroupNorm(groups, eps)(f) with weight gn_weight and bias gn_bias [C]; with swish, x * sigmoid(x) of that.  f [B,C,H,W] fp32 /
    fp16 / bf16.  -> `out` (which may be `f` when the types are equal: in place) or a new tensor; fp32 unless out / out_dtype is the
    features' half type.  On finite inputs bit for bit spatial_norm with conv_y = 1 and conv_b = 0.  No autograd."""
    return _forward("group_norm", False, f, None, (gn_weight, gn_bias), groups, eps, swish, out, out_dtype)[0]


def group_norm_train(f, gn_weight, gn_bias, groups=32, eps=1e-6, swish=False, out=None, out_dtype=None):
    """group_norm that also returns what its backward needs besides its inputs: -> (out, stats), out bit for bit group_norm's, stats
    fp32 [B * groups, 2] = (mean, rstd) of each group (cgic_group_norm_train).  No autograd: torch.ops.cgic.group_norm_train is the
    differentiable form."""
    return _forward("group_norm_train", True, f, None, (gn_weight, gn_bias), groups, eps, swish, out, out_dtype)


GRADS = ("f", "zq", "gn_weight", "gn_bias", "wy", "by", "wb", "bb")
GN_GRADS = ("f", "gn_weight", "gn_bias")


def backward_workspace_bytes(dtype, B, C, H, W, groups=32):
    """bytes of workspace that spatial_norm_backward needs for features of this type and shape (a function of the shape alone)"""
    return int(_lib.lib().cgic_spatial_norm_backward_workspace_bytes(_DT[dtype], B, C, H, W, int(groups)))


def group_norm_backward_workspace_bytes(dtype, B, C, H, W, groups=32):
    """the same for group_norm_backward: two sums per channel and tile instead of twelve, no zq partials"""
    return int(_lib.lib().cgic_group_norm_backward_workspace_bytes(_DT[dtype], B, C, H, W, int(groups)))


def spatial_norm_backward(go, f, zq, stats, gn_weight, gn_bias, wy, by, wb, bb, groups=32, swish=False, need=GRADS, df_dtype=None, outs=None,
                          workspace=None):
    """the gradients of spatial_norm_train's `out` (csrc/cgic_norm_bwd.hip: reduce, finish, apply -- three launches, every sum in
    float64 in a fixed order, no atomics: repeated calls are bit-identical and an image's df and dzq do not depend on its batch).
    go [B,C,H,W]: the gradient of `out`, fp32 or f's half type; f, zq, the parameters, groups, swish: the forward's; stats: its
    second result.  need: the gradients that are wanted, names out of GRADS -- the others are neither computed nor stored.
    -> a tuple in GRADS' order, None where not wanted: df [B,C,H,W] in f's type (df_dtype=torch.float32: fp32; a half df is the fp32
    value rounded once), dzq fp32 [B,4,hq,wq] (exactly 0 where a sub-sampled axis never reads zq), the parameter gradients fp32 in
    the shapes of the parameters.  outs: {name: tensor} to write into (df may be go itself when the types are equal); workspace: a
    uint8 tensor of at least backward_workspace_bytes(...) bytes, 16-byte aligned (it need not be zeroed).
    A NaN in f gives NaN where float64 autograd of the reference's expression gives NaN; +-Inf in f or go is not specified: torch's
    own GroupNorm backward uses another algebra there and the patterns differ legitimately.  No autograd (once-differentiable)."""
    return _backward("spatial_norm_backward", GRADS, go, f, zq, stats, (gn_weight, gn_bias, wy, by, wb, bb), groups, swish, need, df_dtype, outs, workspace)


def group_norm_backward(go, f, stats, gn_weight, gn_bias, groups=32, swish=False, need=GN_GRADS, df_dtype=None, outs=None, workspace=None):
    """the gradients of group_norm_train's `out`: spatial_norm_backward without zq (cgic_group_norm_backward: the same three launches
    with two float64 plane sums per channel; deterministic, batch-independent, no atomics).  need: names out of GN_GRADS.  -> a tuple
    in GN_GRADS' order, None where not wanted: df in f's type (df_dtype=torch.float32: fp32), dgn_weight and dgn_bias fp32 in the
    parameters' shapes.  outs, workspace (group_norm_backward_workspace_bytes(...) bytes): as spatial_norm_backward's.  No autograd."""
    return _backward("group_norm_backward", GN_GRADS, go, f, None, stats, (gn_weight, gn_bias), groups, swish, need, df_dtype, outs, workspace)


def _backward(name, grads, go, f, zq, stats, params, groups, swish, need, df_dtype, outs, workspace):
    """spatial_norm_backward and group_norm_backward (zq None, two parameters): the checks, then the one call of cgic_<name>"""
    plain = zq is None
    outs = dict(outs or {})
    _lib.require_device(f, go, *(() if plain else (zq,)), stats, *params, workspace, *outs.values())
    B, C, H, W, hq, wq, groups = _check_call(name, f, zq, params, groups)
    need = tuple(need)
    if not need or any(n not in grads for n in need) or any(n not in need for n in outs):
        raise ValueError(f"{name}: need {need}, outs {tuple(outs)}; expected names out of {grads}, at least one, outs among the needed")
    if B == 0:
        raise ValueError(f"{name}: an empty batch")
    half = f.dtype if f.dtype != torch.float32 else None
    if tuple(go.shape) != tuple(f.shape) or go.dtype not in (torch.float32, half):
        raise TypeError(f"{name}: go {go.dtype} {tuple(go.shape)}; expected {tuple(f.shape)} in torch.float32" + ("" if half is None else f" or {half}"))
    if tuple(stats.shape) != (B * groups, 2) or stats.dtype != torch.float32:
        raise TypeError(f"{name}: stats {stats.dtype} {tuple(stats.shape)}; expected torch.float32 [{B * groups}, 2] ({name[:-9]}_train's)")
    if df_dtype is None:
        df_dtype = outs["f"].dtype if "f" in outs else f.dtype
    if df_dtype not in (torch.float32, half):
        raise TypeError(f"{name}: df_dtype {df_dtype}; expected torch.float32" + ("" if half is None else f" or the features' {half}"))
    shapes = {"f": (tuple(f.shape), df_dtype), "zq": ((B, ZQ_CHANNELS, hq, wq), torch.float32)}
    for n, p in zip(grads[1 if plain else 2:], params):
        shapes[n] = (tuple(p.shape), torch.float32)
    for n, t in outs.items():
        if tuple(t.shape) != shapes[n][0] or t.dtype != shapes[n][1] or not t.is_contiguous() or t.device != f.device:
            raise ValueError(f"{name}: outs[{n!r}] {t.dtype} {tuple(t.shape)} on {t.device}; expected contiguous {shapes[n][1]} {shapes[n][0]} on {f.device}")
    nbytes = (group_norm_backward_workspace_bytes if plain else backward_workspace_bytes)(f.dtype, B, C, H, W, groups)
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.numel() < nbytes or not workspace.is_contiguous() or workspace.device != f.device):
        raise ValueError(f"{name}: workspace {workspace.dtype} of {workspace.numel()} elements; expected contiguous torch.uint8 of at least {nbytes} on {f.device}")
    f, go, stats = f.contiguous(), go.contiguous(), stats.contiguous()
    params = tuple(p.detach().contiguous().float() for p in params)
    res = {n: outs[n] if n in outs else torch.empty(shapes[n][0], dtype=shapes[n][1], device=f.device) for n in need}
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
    if plain:
        mid = (groups,)
    else:
        zq = zq.contiguous().float()
        mid = (_lib.ptr(zq), hq, wq, groups)
    with _lib.on_device(f.device):
        _lib.call("cgic_" + name, _lib.ptr(f), _DT[f.dtype], _lib.ptr(go), _DT[go.dtype], B, C, H, W, *mid, _lib.ptr(stats), *(_lib.ptr(p) for p in params),
                  int(bool(swish)), _lib.ptr(res.get("f")), _DT[df_dtype], *(_lib.ptr(res.get(n)) for n in grads[1:]), _lib.ptr(workspace),
                  workspace.numel(), _lib.current_stream(f.device))
    return tuple(res.get(n) for n in grads)


@torch.library.custom_op("cgic::spatial_norm", mutates_args=(), device_types="cuda")
def spatial_norm_op(f: torch.Tensor, zq: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, wy: torch.Tensor, by: torch.Tensor,
                    wb: torch.Tensor, bb: torch.Tensor, groups: int, eps: float, swish: bool, half_out: bool) -> torch.Tensor:
    """torch.ops.cgic.spatial_norm: spatial_norm as a custom op (schema, fake kernel; inference only -- the differentiable form is
    torch.ops.cgic.spatial_norm_train below): fp32 [B,C,H,W], or with half_out the type of f"""
    return spatial_norm(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups=groups, eps=eps, swish=swish, out_dtype=f.dtype if half_out else None)


@spatial_norm_op.register_fake
def _(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups, eps, swish, half_out):
    return f.new_empty(f.shape, dtype=f.dtype if half_out else torch.float32)


@torch.library.custom_op("cgic::spatial_norm_train", mutates_args=(), device_types="cuda")
def spatial_norm_train_op(f: torch.Tensor, zq: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, wy: torch.Tensor, by: torch.Tensor,
                          wb: torch.Tensor, bb: torch.Tensor, groups: int, eps: float, swish: bool, half_out: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch.ops.cgic.spatial_norm_train: spatial_norm_train as a custom op (schema, fake kernel, autograd formula): (out, stats).
    The gradient of `out` reaches f, zq and the six parameters through spatial_norm_backward -- as far as each needs one; `stats`
    carries no gradient.  Once-differentiable: a backward under create_graph=True raises."""
    return spatial_norm_train(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups=groups, eps=eps, swish=swish, out_dtype=f.dtype if half_out else None)


@spatial_norm_train_op.register_fake
def _(f, zq, gn_weight, gn_bias, wy, by, wb, bb, groups, eps, swish, half_out):
    return f.new_empty(f.shape, dtype=f.dtype if half_out else torch.float32), f.new_empty((f.shape[0] * groups, 2), dtype=torch.float32)


def _register_train_autograd(op, grads, backward, name, module):
    """the autograd formula of a *_train op whose first len(grads) inputs are the tensors (f first), followed by groups, eps, swish,
    half_out: the gradient of `out` through `backward` (spatial_norm_backward / group_norm_backward) for the inputs that need one"""
    n = len(grads)

    def setup(ctx, inputs, output):
        ctx.save_for_backward(*inputs[:n], output[1])
        ctx.groups, ctx.swish = inputs[n], inputs[n + 2]

    def bwd(ctx, g_out, _g_stats):
        if torch.is_grad_enabled():
            raise RuntimeError(f"cgic::{name}_train is once-differentiable: its backward (cgic_{name}_backward) has no autograd formula, "
                               f"so a backward under create_graph=True (a double backward) is not available; {module}.backward_kernel = False "
                               "takes torch's expression, which can be differentiated twice")
        *inputs, stats = ctx.saved_tensors
        need = tuple(g for g, want in zip(grads, ctx.needs_input_grad[:n]) if want)
        if g_out is None or not need:
            return (None,) * (n + 4)
        f = inputs[0]
        if g_out.dtype != torch.float32 and g_out.dtype != f.dtype:
            g_out = g_out.float()
        res = backward(g_out, stats=stats, **dict(zip(grads, inputs)), groups=ctx.groups, swish=ctx.swish, need=need)     # (the names are its parameters')
        return (*(None if g is None else g.to(t.dtype) for g, t in zip(res, inputs)), None, None, None, None)

    op.register_autograd(bwd, setup_context=setup)


_register_train_autograd(spatial_norm_train_op, GRADS, spatial_norm_backward, "spatial_norm", "SpatialNorm")


@torch.library.custom_op("cgic::group_norm", mutates_args=(), device_types="cuda")
def group_norm_op(f: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, groups: int, eps: float, swish: bool, half_out: bool) -> torch.Tensor:
    """torch.ops.cgic.group_norm: group_norm as a custom op (schema, fake kernel; inference only -- the differentiable form is
    torch.ops.cgic.group_norm_train below): fp32 [B,C,H,W], or with half_out the type of f"""
    return group_norm(f, gn_weight, gn_bias, groups=groups, eps=eps, swish=swish, out_dtype=f.dtype if half_out else None)


@group_norm_op.register_fake
def _(f, gn_weight, gn_bias, groups, eps, swish, half_out):
    return f.new_empty(f.shape, dtype=f.dtype if half_out else torch.float32)


@torch.library.custom_op("cgic::group_norm_train", mutates_args=(), device_types="cuda")
def group_norm_train_op(f: torch.Tensor, gn_weight: torch.Tensor, gn_bias: torch.Tensor, groups: int, eps: float, swish: bool,
                        half_out: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch.ops.cgic.group_norm_train: group_norm_train as a custom op (schema, fake kernel, autograd formula): (out, stats).  The
    gradient of `out` reaches f and the two parameters through group_norm_backward -- as far as each needs one; `stats` carries no
    gradient.  Once-differentiable: a backward under create_graph=True raises."""
    return group_norm_train(f, gn_weight, gn_bias, groups=groups, eps=eps, swish=swish, out_dtype=f.dtype if half_out else None)


@group_norm_train_op.register_fake
def _(f, gn_weight, gn_bias, groups, eps, swish, half_out):
    return f.new_empty(f.shape, dtype=f.dtype if half_out else torch.float32), f.new_empty((f.shape[0] * groups, 2), dtype=torch.float32)


_register_train_autograd(group_norm_train_op, GN_GRADS, group_norm_backward, "group_norm", "GroupNorm")


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
    with torch ops -- unless `backward_kernel` is set: then a call that needs a gradient and meets the other conditions runs the
    library's training forward and, in the backward pass, its backward kernels (with add_conv, torch's interpolate and 3x3 conv stay
    in front with their own autograd and receive the kernel's dzq)."""

    #: True: a call that needs a gradient and that the kernel could serve goes through torch.ops.cgic.spatial_norm_train, whose
    #: backward is the library's (spatial_norm_backward), instead of torch's expression.  A class attribute, so that adopt(), which
    #: bypasses __init__, has it too; set it on an instance (patch_norms(model, backward_kernel=True)) or on the class.
    backward_kernel = False

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
        """the inference kernel serves this call (otherwise: the training kernels if `backward_kernel` is set and they can, else the
        reference's expression in torch ops)"""
        return self._route(f, zq) == "kernel"

    def uses_backward_kernel(self, f, zq):
        """the call needs a gradient, `backward_kernel` is set and the training kernels (forward with statistics, backward) serve it.
        An empty batch stays on torch's path, whose backward returns empty gradients"""
        return self._route(f, zq) == "train"

    def _route(self, f, zq):
        """"kernel" (inference), "train" (forward with statistics + backward kernels) or "torch": every condition looked at once"""
        gn = self.norm_layer
        if not (f.is_cuda and zq.is_cuda and f.dim() == 4 and zq.dim() == 4 and f.dtype in _DT and zq.dtype in _DT):
            return "torch"
        if not (isinstance(gn, torch.nn.GroupNorm) and gn.affine and gn.num_channels == f.shape[1] and self.conv_y.out_channels == f.shape[1]):
            return "torch"
        if zq.shape[1] != ZQ_CHANNELS or self.conv_y.in_channels != ZQ_CHANNELS or zq.shape[0] != f.shape[0]:
            return "torch"
        if self.conv_y.bias is None or self.conv_b.bias is None:
            return "torch"
        needs_grad = torch.is_grad_enabled() and (f.requires_grad or zq.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad and not (self.backward_kernel and f.shape[0] > 0):
            return "torch"
        if not (self.add_conv or (integer_ratio(f.shape[2], zq.shape[2]) and integer_ratio(f.shape[3], zq.shape[3]))):
            return "torch"
        return "train" if needs_grad else "kernel"

    def forward(self, f, zq, swish=False, out_dtype=None):
        route = self._route(f, zq)
        train = route == "train"
        if route != "torch":
            if self.add_conv:                   # the 3x3 conv works on the interpolated zq: both stay torch's, the kernel runs at ratio 1
                zq = self.conv(torch.nn.functional.interpolate(zq, size=f.shape[-2:], mode="nearest"))
            gn = self.norm_layer
            half = out_dtype is not None and out_dtype != torch.float32
            if half and out_dtype != f.dtype:
                raise TypeError(f"SpatialNorm: out_dtype {out_dtype}; expected torch.float32 or the features' {f.dtype}")
            args = (f, zq, gn.weight, gn.bias, self.conv_y.weight, self.conv_y.bias, self.conv_b.weight, self.conv_b.bias, gn.num_groups, gn.eps,
                    bool(swish), half)
            return torch.ops.cgic.spatial_norm_train(*args)[0] if train else torch.ops.cgic.spatial_norm(*args)
        zq = torch.nn.functional.interpolate(zq, size=f.shape[-2:], mode="nearest")
        if self.add_conv:
            zq = self.conv(zq)
        new_f = self.norm_layer(f) * self.conv_y(zq) + self.conv_b(zq)
        if swish:
            new_f = new_f * torch.sigmoid(new_f)
        return new_f if out_dtype is None else new_f.to(out_dtype)


def patch_norms(model, backward_kernel=False):
    """swap every module of `model` that has the reference SpatialNorm's shape for norm.SpatialNorm on the same submodules;
    -> the number swapped.  backward_kernel=True also sets SpatialNorm.backward_kernel on every norm.SpatialNorm of the model (those
    swapped earlier included): calls that need a gradient then run the library's forward and backward kernels"""
    found = [(parent, name) for parent in model.modules() for name, child in parent.named_children()
             if not isinstance(child, SpatialNorm) and has_reference_shape(child)]
    for parent, name in found:
        setattr(parent, name, SpatialNorm.adopt(getattr(parent, name)))
    if backward_kernel:
        for m in model.modules():
            if isinstance(m, SpatialNorm):
                m.backward_kernel = True
    return len(found)


class GroupNorm(torch.nn.GroupNorm):
    """torch.nn.GroupNorm -- the encoder's Normalize (vqvae_blocks.py:34) -- on the library's kernel: a subclass, so isinstance
    checks, the state_dict keys (weight, bias) and SpatialNorm's / AttnBlock's handling of a GroupNorm stay what they are.
    forward(x) is torch's; forward(x, swish=True) also applies the swish that ResnetBlock and the encoder's norm_out heads put behind
    it (vqvae_blocks.py:119-120).  The kernel serves the call when x is a fp32 / fp16 / bf16 [B,C,H,W] on the device, the norm is
    affine and no autograd is needed; anything else is F.group_norm (and x * sigmoid(x)) -- unless `backward_kernel` is set: then
    a call that needs a gradient runs the library's training forward and, in the backward pass, its backward kernels.
    The result of half features is fp32 under torch.autocast (where F.group_norm, on autocast's fp32 list, returns fp32 too) and the
    features' type otherwise, as torch's; out_dtype overrides it: the same fp32 value rounded once."""

    #: as SpatialNorm.backward_kernel: calls that need a gradient go through torch.ops.cgic.group_norm_train
    backward_kernel = False

    @classmethod
    def adopt(cls, module):
        """a GroupNorm on the SAME parameter objects as `module` (a torch.nn.GroupNorm)"""
        if not isinstance(module, torch.nn.GroupNorm):
            raise TypeError(f"GroupNorm.adopt: {type(module).__name__} is not a torch.nn.GroupNorm")
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.num_groups, m.num_channels, m.eps, m.affine = module.num_groups, module.num_channels, module.eps, module.affine
        m.register_parameter("weight", module.weight)
        m.register_parameter("bias", module.bias)
        m.train(module.training)
        return m

    def uses_kernel(self, x):
        """the inference kernel serves this call"""
        return self._route(x) == "kernel"

    def uses_backward_kernel(self, x):
        """the call needs a gradient, `backward_kernel` is set and the training kernels serve it"""
        return self._route(x) == "train"

    def _route(self, x):
        """"kernel" (inference), "train" (forward with statistics + backward kernels) or "torch", as SpatialNorm._route"""
        if not (x.is_cuda and x.dim() == 4 and x.dtype in _DT):
            return "torch"
        if not (self.affine and self.num_channels == x.shape[1] and self.weight.is_cuda):
            return "torch"
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad and not (self.backward_kernel and x.shape[0] > 0):
            return "torch"
        return "train" if needs_grad else "kernel"

    def forward(self, x, swish=False, out_dtype=None):
        route = self._route(x)
        if route != "torch":
            if out_dtype is None:
                half = x.dtype != torch.float32 and not torch.is_autocast_enabled("cuda")
            else:
                half = out_dtype != torch.float32
                if half and out_dtype != x.dtype:
                    raise TypeError(f"GroupNorm: out_dtype {out_dtype}; expected torch.float32 or the features' {x.dtype}")
            args = (x, self.weight, self.bias, self.num_groups, self.eps, bool(swish), half)
            return torch.ops.cgic.group_norm_train(*args)[0] if route == "train" else torch.ops.cgic.group_norm(*args)
        h = torch.nn.functional.group_norm(x, self.num_groups, self.weight, self.bias, self.eps)
        if swish:
            h = h * torch.sigmoid(h)
        return h if out_dtype is None else h.to(out_dtype)


def patch_group_norms(model, backward_kernel=False):
    """swap every affine torch.nn.GroupNorm of `model` for norm.GroupNorm on the same parameters -- except the norm_layer of a
    SpatialNorm-shaped module, which that module's own kernel reads; -> the number swapped.  backward_kernel=True also sets
    GroupNorm.backward_kernel on those swapped in by this call"""
    found = [(parent, name) for parent in model.modules() for name, child in parent.named_children()
             if isinstance(child, torch.nn.GroupNorm) and not isinstance(child, GroupNorm) and child.affine
             and not (name == "norm_layer" and (isinstance(parent, SpatialNorm) or has_reference_shape(parent)))]
    for parent, name in found:
        m = GroupNorm.adopt(getattr(parent, name))
        if backward_kernel:
            m.backward_kernel = True
        setattr(parent, name, m)
    return len(found)
