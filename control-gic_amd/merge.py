"""The mask-merge kernels either side of the quantiser (vqvae_blocks.py:361-366, decoder.py:304-305,366-378): the raw calls with
their checks, no autograd.  torch.ops.cgic.grain_merge / avg_pool / decoder_blend_* wrap them (ops.py: schema, fake kernel,
autograd formula); model.decoder_blend_*(..., out=) call them directly.  The masks are the router's int32 tensors.

Feature types.  fp32 features take the _f32 kernels.  Features that are ALL fp16 or ALL bf16 (the conv nets under torch.autocast)
take the _h calls (csrc/cgic_merge.hip: the same kernels), which read the halves themselves: no cast pass.  Any mixture of types is cast to
fp32 first, as every type was before the _h kernels existed.  The result is fp32 -- what the reference's expressions promote to,
the masks being .float() -- unless `out_dtype` (or the dtype of `out`) asks for the features' own half type: the same fp32 value
rounded once to nearest-even, an option the reference does not have.
"""
import torch

from . import _lib

_DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}          # CGIC_DT_* (include/cgic_hip.h)


def _half_type(*feats):
    """the fp16 / bf16 type all features share, or None: the fp32 path (fp32 as it is, any mixture through a cast)"""
    dt = feats[0].dtype
    return dt if dt in (torch.float16, torch.bfloat16) and all(t.dtype == dt for t in feats) else None


def _features(half, *feats):
    return tuple(t.contiguous() if half is not None else t.contiguous().float() for t in feats)


def _result_type(name, half, out_dtype, out=None):
    """the dtype of the result: fp32, or the features' half type when `out_dtype` / the dtype of `out` says so"""
    if out is not None:
        if out.dtype != torch.float32 and (half is None or out.dtype != half):
            raise TypeError(f"{name}: out is {out.dtype}; the result of these features is torch.float32" if half is None else
                            f"{name}: out is {out.dtype}; expected torch.float32 or the features' {half}")
        if out_dtype is not None and out_dtype != out.dtype:
            raise TypeError(f"{name}: out_dtype {out_dtype}, but out is {out.dtype}")
        return out.dtype
    if out_dtype is None or out_dtype == torch.float32:
        return torch.float32
    if half is None or out_dtype != half:
        raise TypeError(f"{name}: out_dtype {out_dtype}; expected torch.float32" + ("" if half is None else f" or the features' {half}")
                        + (" (the features are not all of one half type)" if half is None else ""))
    return half


def _checked_out(name, h, out):
    """`out=` of a blend: a contiguous tensor of h's shape on h's device (its dtype: _result_type)"""
    if out.device != h.device:
        raise ValueError(f"{name}: out is on {out.device}, h on {h.device}")
    if tuple(out.shape) != tuple(h.shape):
        raise ValueError(f"{name}: out {tuple(out.shape)} must have h's shape {tuple(h.shape)}")
    if not out.is_contiguous():
        raise ValueError(f"{name}: out must be contiguous")
    return out


def grain_merge(h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f, out_dtype=None):
    """up4(h_coarse)*up4(mask_c) + up2(h_medium)*up2(mask_m) + h_fine*mask_f in one pass (vqvae_blocks.py:361-366), bit-identical"""
    _lib.require_device(h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f)
    half = _half_type(h_coarse, h_medium, h_fine)
    res = _result_type("grain_merge", half, out_dtype)
    hc, hm, hf = _features(half, h_coarse, h_medium, h_fine)
    mc, mm, mf = (m.contiguous() for m in (mask_c, mask_m, mask_f))
    _lib.require_int32_masks(mc, mm, mf)
    B, C, h, w = hf.shape
    if tuple(hc.shape) != (B, C, h // 4, w // 4) or tuple(hm.shape) != (B, C, h // 2, w // 2):
        raise ValueError("h_coarse / h_medium must be the fine map's shape divided by 4 / 2")
    if mc.numel() != B * (h // 4) * (w // 4) or mm.numel() != B * (h // 2) * (w // 2) or mf.numel() != B * h * w:
        raise ValueError("grain_merge: masks at 1/4, 1/2, 1/1 of the fine grid, one per image")
    out = torch.empty_like(hf, dtype=res)
    with _lib.on_device(hf.device):
        if half is None:
            _lib.call("cgic_grain_merge_f32", _lib.ptr(hc), _lib.ptr(hm), _lib.ptr(hf), _lib.ptr(mc), _lib.ptr(mm),
                      _lib.ptr(mf), B, C, h, w, _lib.ptr(out), _lib.current_stream(hf.device))
        else:
            _lib.call("cgic_grain_merge_h", _lib.ptr(hc), _lib.ptr(hm), _lib.ptr(hf), _DT[half], _lib.ptr(mc), _lib.ptr(mm),
                      _lib.ptr(mf), B, C, h, w, _lib.ptr(out), _DT[res], _lib.current_stream(hf.device))
    return out


def avg_pool(x, k, out_dtype=None):
    """torch.nn.AvgPool2d(k, k, 0) for k in (2, 4) (decoder.py:304-305,366-367): row-major window sum / k^2, bit-identical to the CPU
    kernel; H and W must be multiples of k (the decoder's are; cgic_avgpool_f32 refuses anything else).  On a half tensor
    out_dtype=x.dtype is what AvgPool2d returns: the fp32 sum / k^2, rounded once"""
    _lib.require_device(x)
    half = _half_type(x)
    res = _result_type("avg_pool", half, out_dtype)
    x, = _features(half, x)
    B, C, H, W = x.shape
    out = torch.empty((B, C, H // k, W // k), dtype=res, device=x.device)
    with _lib.on_device(x.device):
        if half is None:
            _lib.call("cgic_avgpool_f32", _lib.ptr(x), B * C, H, W, int(k), _lib.ptr(out), _lib.current_stream(x.device))
        else:
            _lib.call("cgic_avgpool_h", _lib.ptr(x), _DT[half], B * C, H, W, int(k), _lib.ptr(out), _DT[res], _lib.current_stream(x.device))
    return out


def decoder_blend_medium(h, h_medium, mask_c, mask_m, refusal, out=None, out_dtype=None):
    """h * up2(mask_c) + h_medium * mask_m on the medium grid (decoder.py:372-374) -> `out` (which may be `h`: in place), or a
    new tensor.  refusal: the caller's words for shapes that do not fit (each names the masks as its own signature does; the
    fine blend's two callers say the same, so its text lives here)"""
    _lib.require_device(h, h_medium, mask_c, mask_m)
    half = _half_type(h, h_medium)
    given = h
    h, hm = _features(half, h, h_medium)
    mc, mm = mask_c.contiguous(), mask_m.contiguous()
    _lib.require_int32_masks(mc, mm)
    B, C, hh, ww = h.shape
    if tuple(hm.shape) != (B, C, hh, ww) or mc.numel() != B * (hh // 2) * (ww // 2) or mm.numel() != B * hh * ww:
        raise ValueError(refusal)
    if out is not None:
        out = _checked_out("decoder_blend_medium", given, out)
    res = _result_type("decoder_blend_medium", half, out_dtype, out)
    if out is None:
        out = torch.empty_like(h, dtype=res)
    with _lib.on_device(h.device):
        if half is None:
            _lib.call("cgic_decoder_blend_medium_f32", _lib.ptr(h), _lib.ptr(hm), _lib.ptr(mc), _lib.ptr(mm), B, C, hh, ww,
                      _lib.ptr(out), _lib.current_stream(h.device))
        else:
            _lib.call("cgic_decoder_blend_medium_h", _lib.ptr(h), _lib.ptr(hm), _DT[half], _lib.ptr(mc), _lib.ptr(mm), B, C, hh, ww,
                      _lib.ptr(out), _DT[res], _lib.current_stream(h.device))
    return out


def decoder_blend_fine(h, h_fine, mask_c, mask_m, mask_f, out=None, out_dtype=None):
    """h * up4(mask_c) + h * up2(mask_m) + h_fine * mask_f on the fine grid (decoder.py:375-378) -> `out` (in place if `out is h`),
    or a new tensor"""
    _lib.require_device(h, h_fine, mask_c, mask_m, mask_f)
    half = _half_type(h, h_fine)
    given = h
    h, hf = _features(half, h, h_fine)
    mc, mm, mf = (m.contiguous() for m in (mask_c, mask_m, mask_f))
    _lib.require_int32_masks(mc, mm, mf)
    B, C, hh, ww = h.shape
    if tuple(hf.shape) != (B, C, hh, ww) or mc.numel() != B * (hh // 4) * (ww // 4) or mm.numel() != B * (hh // 2) * (ww // 2) \
            or mf.numel() != B * hh * ww:
        raise ValueError("decoder_blend_fine: h, h_fine on the fine grid; masks at 1/4, 1/2, 1/1 of it")
    if out is not None:
        out = _checked_out("decoder_blend_fine", given, out)
    res = _result_type("decoder_blend_fine", half, out_dtype, out)
    if out is None:
        out = torch.empty_like(h, dtype=res)
    with _lib.on_device(h.device):
        if half is None:
            _lib.call("cgic_decoder_blend_fine_f32", _lib.ptr(h), _lib.ptr(hf), _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf), B, C, hh, ww,
                      _lib.ptr(out), _lib.current_stream(h.device))
        else:
            _lib.call("cgic_decoder_blend_fine_h", _lib.ptr(h), _lib.ptr(hf), _DT[half], _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf), B, C,
                      hh, ww, _lib.ptr(out), _DT[res], _lib.current_stream(h.device))
    return out
