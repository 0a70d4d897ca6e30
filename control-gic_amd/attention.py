"""AttnBlock's attention (CGIC/modules/vqvae/decoder.py:189-213, vqvae_blocks.py:168-193) on the library's kernel
(csrc/cgic_attn.hip):

    w_ = torch.bmm(q.permute(0, 2, 1), k) * int(c) ** (-0.5)       # [B, N, N]
    w_ = softmax(w_, dim=2)
    h_ = torch.bmm(v, w_.permute(0, 2, 1))                          # [B, C, N]

one head as wide as the channel count, computed flash-style: the [B, N, N] matrix never exists in memory.  `attention` is the raw
call with its checks (no autograd) and the one function that reaches cgic_attention; torch.ops.cgic.attention wraps it
(attention_op below: schema and fake kernel).  For training, `attention_backward` is the raw call of the backward kernels
(csrc/cgic_attn_bwd.hip: the gradients of q, k, v from the forward's out and lse, again without the matrix; the one function that
reaches cgic_attention_backward) and torch.ops.cgic.attention_train the differentiable op on the two.  `AttnBlock` is the module with the reference's constructors and state_dict keys,
which model.install(..., patch_attention=True) puts in the place of the reference's.

Types.  fp32 q, k, v are multiplied as fp32.  fp16 / bf16 (the 1x1 convs under torch.autocast) are read as they are; the scores,
the softmax and the accumulator are fp32 where torch's half bmm rounds the scores to the half type.  The result has the inputs'
type unless out / out_dtype says fp32: under autocast the reference's second bmm returns the half type, and so does this.
"""
from typing import Tuple

import torch

from . import _lib

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}          # CGIC_DT_* (include/cgic_hip.h)


def supported(in_dtype, out_dtype, B, C, N):
    """cgic_attention_supported: the kernel is built for these types and this shape (True / False; raises for arguments that are
    wrong in themselves)"""
    if in_dtype not in _DT or out_dtype not in _DT:
        return False
    return bool(_lib.call("cgic_attention_supported", _DT[in_dtype], _DT[out_dtype], int(B), int(C), int(N)))


def _images(t, B, C, N):
    """`t` [B,C,N] or [B,C,H,W] as the kernel reads it -- every image [C, N] with the tokens contiguous, images a constant stride
    apart -- and that stride in elements; a copy only where the layout is another"""
    inner = t.stride(-1) == 1 and (t.dim() == 3 or t.stride(2) == t.shape[3]) and t.stride(1) == N
    if not inner or (B > 1 and t.stride(0) < C * N):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else C * N)


def attention(q, k, v, scale=None, out=None, out_dtype=None, lse=False):
    """softmax(scale * q^T k) applied to v.  q, k, v [B,C,N] or [B,C,H,W] (N = H * W) of one type (fp32, fp16 or bf16) and shape; views
    of one [B,3C,N] tensor are read where they lie.  scale: int(C) ** -0.5 by default, as the reference.  -> `out` or a new tensor
    of q's shape, of the inputs' type unless out / out_dtype says torch.float32; with lse=True also the fp32 [B,N] log-sum-exp of
    the scaled scores.  No autograd."""
    _lib.require_device(q, k, v, out)
    if q.dim() not in (3, 4) or q.dtype not in _DT:
        raise TypeError(f"attention: q {q.dtype} {tuple(q.shape)}; expected fp32, fp16 or bf16 [B,C,N] or [B,C,H,W]")
    for name, t in (("k", k), ("v", v)):
        if t.dtype != q.dtype or tuple(t.shape) != tuple(q.shape) or t.device != q.device:
            raise ValueError(f"attention: {name} {t.dtype} {tuple(t.shape)} on {t.device}; q is {q.dtype} {tuple(q.shape)} on {q.device}")
    B, C = q.shape[0], q.shape[1]
    N = q.shape[2] if q.dim() == 3 else q.shape[2] * q.shape[3]
    if N < 1 or C < 1:
        raise ValueError(f"attention: q {tuple(q.shape)}: no tokens or no channels")
    if out is not None:
        if out.device != q.device or tuple(out.shape) != tuple(q.shape) or not out.is_contiguous():
            raise ValueError(f"attention: out {tuple(out.shape)} on {out.device} must be contiguous, of q's shape {tuple(q.shape)} and on {q.device}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError(f"attention: out_dtype {out_dtype}, but out is {out.dtype}")
        out_dtype = out.dtype
    res = q.dtype if out_dtype is None else out_dtype
    if res != q.dtype and res != torch.float32:
        raise TypeError(f"attention: result type {res}; expected the inputs' {q.dtype} or torch.float32")
    scale = int(C) ** (-0.5) if scale is None else float(scale)
    (q_, qs), (k_, ks), (v_, vs) = (_images(t.detach(), B, C, N) for t in (q, k, v))
    if out is None:
        out = torch.empty(q.shape, dtype=res, device=q.device)
    lse_t = torch.empty((B, N), dtype=torch.float32, device=q.device) if lse else None
    nbytes = _lib.lib().cgic_attention_workspace_bytes(_DT[q.dtype], B, C, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device) if nbytes else None
    with _lib.on_device(q.device):
        _lib.call("cgic_attention", _lib.ptr(q_), _lib.ptr(k_), _lib.ptr(v_), _DT[q.dtype], B, C, N, qs, ks, vs, scale, _lib.ptr(out), _DT[res],
                  _lib.ptr(lse_t), _lib.ptr(ws), nbytes, _lib.current_stream(q.device))
    return (out, lse_t) if lse else out


GRADS = ("dq", "dk", "dv")


def backward_supported(in_dtype, grad_dtype, B, C, N):
    """cgic_attention_backward_supported: the backward kernels are built for these types and this shape (True / False)"""
    if in_dtype not in _DT or grad_dtype not in _DT:
        return False
    return bool(_lib.call("cgic_attention_backward_supported", _DT[in_dtype], _DT[grad_dtype], int(B), int(C), int(N)))


def backward_workspace_bytes(dtype, B, C, N):
    """bytes of workspace that attention_backward needs for inputs of this type and shape (a function of the shape alone: delta)"""
    return int(_lib.lib().cgic_attention_backward_workspace_bytes(_DT[dtype], int(B), int(C), int(N)))


def attention_backward(go, q, k, v, out, lse, scale=None, need=GRADS, grad_dtype=None, outs=None, workspace=None):
    """the gradients of attention's result (csrc/cgic_attn_bwd.hip: delta, a query-owning launch for dq, a key-owning launch for dk
    and dv; P and dS recomputed per tile, no tokens x tokens tensor, no atomics: repeated calls are bit-identical and an image's
    gradients do not depend on its batch).  go: the gradient of `out`, of the inputs' type and shape; q, k, v, scale: the forward's;
    out, lse: what attention(q, k, v, scale, lse=True) returned, out in the inputs' type.  need: the gradients that are wanted, names
    out of GRADS -- the others are neither computed nor stored.  -> (dq, dk, dv), None where not wanted, each of q's shape in the
    inputs' type (grad_dtype=torch.float32: fp32; a half gradient is the fp32 value rounded once).  outs: {name: tensor} to write
    into (contiguous, of q's shape); workspace: a uint8 tensor of at least backward_workspace_bytes(...) bytes, 16-byte aligned (it
    need not be zeroed).
    A NaN reaches the elements it reaches under float64 autograd of the reference's expression; +-Inf in an input and rows whose lse
    is not finite are not specified.  No autograd (once-differentiable)."""
    name = "attention_backward"
    outs = dict(outs or {})
    _lib.require_device(go, q, k, v, out, lse, workspace, *outs.values())
    if q.dim() not in (3, 4) or q.dtype not in _DT:
        raise TypeError(f"{name}: q {q.dtype} {tuple(q.shape)}; expected fp32, fp16 or bf16 [B,C,N] or [B,C,H,W]")
    for tname, t in (("go", go), ("k", k), ("v", v), ("out", out)):
        if t.dtype != q.dtype or tuple(t.shape) != tuple(q.shape) or t.device != q.device:
            raise ValueError(f"{name}: {tname} {t.dtype} {tuple(t.shape)} on {t.device}; q is {q.dtype} {tuple(q.shape)} on {q.device}")
    B, C = q.shape[0], q.shape[1]
    N = q.shape[2] if q.dim() == 3 else q.shape[2] * q.shape[3]
    if N < 1 or C < 1:
        raise ValueError(f"{name}: q {tuple(q.shape)}: no tokens or no channels")
    if B == 0:
        raise ValueError(f"{name}: an empty batch")
    if lse.dtype != torch.float32 or tuple(lse.shape) != (B, N) or lse.device != q.device:
        raise TypeError(f"{name}: lse {lse.dtype} {tuple(lse.shape)} on {lse.device}; expected torch.float32 [{B}, {N}] on {q.device} (attention(..., lse=True)'s)")
    need = tuple(need)
    if not need or any(n not in GRADS for n in need) or len(set(need)) != len(need) or any(n not in need for n in outs):
        raise ValueError(f"{name}: need {need}, outs {tuple(outs)}; expected names out of {GRADS}, at least one, each once, outs among the needed")
    if grad_dtype is None:
        grad_dtype = next(iter(outs.values())).dtype if outs else q.dtype
    if grad_dtype != q.dtype and grad_dtype != torch.float32:
        raise TypeError(f"{name}: grad_dtype {grad_dtype}; expected the inputs' {q.dtype} or torch.float32")
    scale = int(C) ** (-0.5) if scale is None else float(scale)
    (go_, gs), (q_, qs), (k_, ks), (v_, vs) = (_images(t.detach(), B, C, N) for t in (go, q, k, v))
    out_, lse_ = out.detach().contiguous(), lse.detach().contiguous()
    for n, t in outs.items():
        if tuple(t.shape) != tuple(q.shape) or t.dtype != grad_dtype or not t.is_contiguous() or t.device != q.device:
            raise ValueError(f"{name}: outs[{n!r}] {t.dtype} {tuple(t.shape)} on {t.device}; expected contiguous {grad_dtype} {tuple(q.shape)} on {q.device}")
    nbytes = backward_workspace_bytes(q.dtype, B, C, N)
    ws = workspace
    if ws is not None and (ws.dtype != torch.uint8 or ws.numel() < nbytes or not ws.is_contiguous() or ws.device != q.device):
        raise ValueError(f"{name}: workspace {ws.dtype} of {ws.numel()} elements; expected contiguous torch.uint8 of at least {nbytes} on {q.device}")
    res = {n: outs[n] if n in outs else torch.empty(q.shape, dtype=grad_dtype, device=q.device) for n in need}
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    with _lib.on_device(q.device):
        _lib.call("cgic_attention_backward", _lib.ptr(go_), _lib.ptr(q_), _lib.ptr(k_), _lib.ptr(v_), _lib.ptr(out_), _lib.ptr(lse_), _DT[q.dtype], B, C, N,
                  gs, qs, ks, vs, scale, *(_lib.ptr(res.get(n)) for n in GRADS), _DT[grad_dtype], _lib.ptr(ws), ws.numel(), _lib.current_stream(q.device))
    return tuple(res.get(n) for n in GRADS)


@torch.library.custom_op("cgic::attention", mutates_args=(), device_types="cuda")
def attention_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, f32_out: bool) -> torch.Tensor:
    """torch.ops.cgic.attention: attention as a custom op (schema, fake kernel; inference only -- the differentiable form is
    torch.ops.cgic.attention_train below): q's shape, of q's type or with f32_out fp32"""
    return attention(q, k, v, scale=scale, out_dtype=torch.float32 if f32_out else None)


@attention_op.register_fake
def _(q, k, v, scale, f32_out):
    return q.new_empty(q.shape, dtype=torch.float32 if f32_out else q.dtype)


@torch.library.custom_op("cgic::attention_train", mutates_args=(), device_types="cuda")
def attention_train_op(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """torch.ops.cgic.attention_train: attention(..., lse=True) as a custom op (schema, fake kernel, autograd formula): (out, lse),
    out of q's type and shape -- the same kernel and bits as torch.ops.cgic.attention.  The gradient of `out` reaches q, k and v
    through attention_backward, as far as each needs one; `lse` is marked non-differentiable (it does not require grad).  Once-differentiable: a backward under
    create_graph=True raises."""
    return attention(q, k, v, scale=scale, lse=True)


@attention_train_op.register_fake
def _(q, k, v, scale):
    n = q.shape[2] if q.dim() == 3 else q.shape[2] * q.shape[3]
    return q.new_empty(q.shape), q.new_empty((q.shape[0], n), dtype=torch.float32)


def _train_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:3], *output)
    ctx.scale = inputs[3]
    ctx.mark_non_differentiable(output[1])          # lse: a loss built on it gets "does not require grad", not a gradient that is short


def _train_bwd(ctx, g_out, _g_lse):
    if torch.is_grad_enabled():
        raise RuntimeError("cgic::attention_train is once-differentiable: its backward (cgic_attention_backward) has no autograd formula, "
                           "so a backward under create_graph=True (a double backward) is not available; AttnBlock.backward_kernel = False "
                           "takes torch's expression, which can be differentiated twice")
    q, k, v, out, lse = ctx.saved_tensors
    need = tuple(n for n, want in zip(GRADS, ctx.needs_input_grad[:3]) if want)
    if g_out is None or not need:
        return (None,) * 4
    if g_out.dtype != q.dtype:
        g_out = g_out.to(q.dtype)
    return (*attention_backward(g_out, q, k, v, out, lse, scale=ctx.scale, need=need), None)


attention_train_op.register_autograd(_train_bwd, setup_context=_train_setup)


def _conv1x1(c, n):
    return (isinstance(c, torch.nn.Conv2d) and c.kernel_size == (1, 1) and c.stride == (1, 1) and c.padding == (0, 0) and c.groups == 1
            and c.in_channels == n and c.out_channels == n)


def has_reference_shape(m):
    """`m` has the members of the reference's AttnBlock (decoder.py:161-213, vqvae_blocks.py:140-192): in_channels, norm, and the
    four 1x1 convs q, k, v, proj_out of that width"""
    n = getattr(m, "in_channels", None)
    return (isinstance(n, int) and isinstance(getattr(m, "norm", None), torch.nn.Module)
            and all(_conv1x1(getattr(m, name, None), n) for name in ("q", "k", "v", "proj_out")))


def _norm_takes_zq(norm):
    from . import norm as _norm
    return isinstance(norm, _norm.SpatialNorm) or _norm.has_reference_shape(norm)


class AttnBlock(torch.nn.Module):
    """the reference's AttnBlock with its constructors and state_dict keys (norm.*, q.*, k.*, v.*, proj_out.*):
    AttnBlock(in_channels) is the encoder's (vqvae_blocks.py:140-192: a GroupNorm, forward(x));
    AttnBlock(in_channels, zq_ch, add_conv) the decoder's (decoder.py:161-213: a SpatialNorm, forward(x, zq)).
    The kernel serves the attention when q, k, v are on the device, no autograd is needed and the library is built for the type
    and shape (cgic_attention_supported); anything else evaluates the reference's expression with torch ops -- unless
    `backward_kernel` is set: then a call that needs a gradient and meets the other conditions runs the same forward kernel with
    its lse and, in the backward pass, the library's backward kernels, and no [B,N,N] tensor is kept for the backward pass either.
    The norm, the four 1x1 convs and the residual add are torch's either way."""

    #: True: an attention that needs a gradient and that the kernels could serve goes through torch.ops.cgic.attention_train, whose
    #: backward is the library's (attention_backward), instead of torch's expression.  A class attribute, so that adopt(), which
    #: bypasses __init__, has it too; set it on an instance (patch_attention(model, backward_kernel=True)) or on the class.
    backward_kernel = False

    def __init__(self, in_channels, zq_ch=None, add_conv=False):
        super().__init__()
        from .norm import SpatialNorm
        self.in_channels = in_channels
        if zq_ch is None:
            self.norm = torch.nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)
        else:
            self.norm = SpatialNorm(in_channels, zq_ch, norm_layer=torch.nn.GroupNorm, freeze_norm_layer=False, add_conv=add_conv,
                                    num_groups=32, eps=1e-6, affine=True)
        for name in ("q", "k", "v", "proj_out"):
            setattr(self, name, torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0))

    @classmethod
    def adopt(cls, module):
        """an AttnBlock on the SAME submodules as `module` (a reference AttnBlock of either kind): the parameter objects and the
        state_dict keys stay what they are"""
        if not has_reference_shape(module):
            raise TypeError(f"AttnBlock.adopt: {type(module).__name__} has not the reference's in_channels / norm / 1x1 q, k, v, proj_out")
        m = cls.__new__(cls)
        torch.nn.Module.__init__(m)
        m.in_channels = module.in_channels
        m.norm = module.norm
        m.q, m.k, m.v, m.proj_out = module.q, module.k, module.v, module.proj_out
        m.train(module.training)
        return m

    def uses_kernel(self, q, k, v):
        """the inference kernel serves this attention (otherwise: the training kernels if `backward_kernel` is set and they can,
        else the reference's expression in torch ops)"""
        return self._route(q, k, v) == "kernel"

    def uses_backward_kernel(self, q, k, v):
        """the attention needs a gradient, `backward_kernel` is set and the kernels (the forward with lse, the backward) serve it.
        An empty batch stays on torch's path, whose backward returns empty gradients"""
        return self._route(q, k, v) == "train"

    def _route(self, q, k, v):
        """"kernel" (inference), "train" (forward with lse + backward kernels) or "torch": every condition looked at once"""
        if not (q.is_cuda and k.is_cuda and v.is_cuda and q.dim() == 4 and q.dtype in _DT and k.dtype == q.dtype and v.dtype == q.dtype):
            return "torch"
        needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
        if needs_grad and not (self.backward_kernel and q.shape[0] > 0):
            return "torch"
        B, C, N = q.shape[0], q.shape[1], q.shape[2] * q.shape[3]
        if not supported(q.dtype, q.dtype, B, C, N) or (needs_grad and not backward_supported(q.dtype, q.dtype, B, C, N)):
            return "torch"
        return "train" if needs_grad else "kernel"

    def forward(self, x, zq=None):
        h_ = self.norm(x, zq) if _norm_takes_zq(self.norm) else self.norm(x)
        q, k, v = self.q(h_), self.k(h_), self.v(h_)
        b, c, h, w = q.shape
        route = self._route(q, k, v)
        if route == "kernel":
            h_ = torch.ops.cgic.attention(q, k, v, int(c) ** (-0.5), False)
        elif route == "train":
            h_ = torch.ops.cgic.attention_train(q, k, v, int(c) ** (-0.5))[0]
        else:
            w_ = torch.bmm(q.reshape(b, c, h * w).permute(0, 2, 1), k.reshape(b, c, h * w))
            w_ = w_ * (int(c) ** (-0.5))
            w_ = torch.nn.functional.softmax(w_, dim=2)
            h_ = torch.bmm(v.reshape(b, c, h * w), w_.permute(0, 2, 1)).reshape(b, c, h, w)
        return x + self.proj_out(h_)


def patch_attention(model, backward_kernel=False):
    """swap every module of `model` that has the reference AttnBlock's shape for attention.AttnBlock on the same submodules;
    -> the number swapped.  backward_kernel=True also sets AttnBlock.backward_kernel on every attention.AttnBlock of the model
    (those swapped earlier included): attentions that need a gradient then run the library's forward and backward kernels.  Off by
    default: the kernels' gradients agree with torch's only within rounding, and they buy memory, not time
    (profiles/attention_backward.md)"""
    found = [(parent, name) for parent in model.modules() for name, child in parent.named_children()
             if not isinstance(child, AttnBlock) and has_reference_shape(child)]
    for parent, name in found:
        setattr(parent, name, AttnBlock.adopt(getattr(parent, name)))
    if backward_kernel:
        for m in model.modules():
            if isinstance(m, AttnBlock):
                m.backward_kernel = True
    return len(found)
