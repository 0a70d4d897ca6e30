"""The mask-merge kernels either side of the quantiser (vqvae_blocks.py:361-366, decoder.py:304-305,366-378): the raw calls with
their checks, no autograd.  torch.ops.cgic.grain_merge / avg_pool / decoder_blend_* wrap them (ops.py: schema, fake kernel,
autograd formula); model.decoder_blend_*(..., out=) call them directly.  The masks are the router's int32 tensors.
"""
import torch

from . import _lib


def grain_merge(h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f):
    """up4(h_coarse)*up4(mask_c) + up2(h_medium)*up2(mask_m) + h_fine*mask_f in one pass (vqvae_blocks.py:361-366), bit-identical"""
    _lib.require_device(h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f)
    hc, hm, hf = (t.contiguous().float() for t in (h_coarse, h_medium, h_fine))
    mc, mm, mf = (m.contiguous() for m in (mask_c, mask_m, mask_f))
    _lib.require_int32_masks(mc, mm, mf)
    B, C, h, w = hf.shape
    if tuple(hc.shape) != (B, C, h // 4, w // 4) or tuple(hm.shape) != (B, C, h // 2, w // 2):
        raise ValueError("h_coarse / h_medium must be the fine map's shape divided by 4 / 2")
    if mc.numel() != B * (h // 4) * (w // 4) or mm.numel() != B * (h // 2) * (w // 2) or mf.numel() != B * h * w:
        raise ValueError("grain_merge: masks at 1/4, 1/2, 1/1 of the fine grid, one per image")
    out = torch.empty_like(hf)
    with _lib.on_device(hf.device):
        _lib.call("cgic_grain_merge_f32", _lib.ptr(hc), _lib.ptr(hm), _lib.ptr(hf), _lib.ptr(mc), _lib.ptr(mm),
                  _lib.ptr(mf), B, C, h, w, _lib.ptr(out), _lib.current_stream(hf.device))
    return out


def avg_pool(x, k):
    """torch.nn.AvgPool2d(k, k, 0) for k in (2, 4) (decoder.py:304-305,366-367): row-major window sum / k^2, bit-identical to the CPU
    kernel; H and W must be multiples of k (the decoder's are; cgic_avgpool_f32 refuses anything else)"""
    _lib.require_device(x)
    x = x.contiguous().float()
    B, C, H, W = x.shape
    out = torch.empty((B, C, H // k, W // k), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.call("cgic_avgpool_f32", _lib.ptr(x), B * C, H, W, int(k), _lib.ptr(out), _lib.current_stream(x.device))
    return out


def decoder_blend_medium(h, h_medium, mask_c, mask_m, refusal, out=None):
    """h * up2(mask_c) + h_medium * mask_m on the medium grid (decoder.py:372-374) -> `out` (which may be `h`: in place), or a
    new tensor.  refusal: the caller's words for shapes that do not fit (each names the masks as its own signature does; the
    fine blend's two callers say the same, so its text lives here)"""
    _lib.require_device(h, h_medium, mask_c, mask_m)
    h, hm = h.contiguous().float(), h_medium.contiguous().float()
    mc, mm = mask_c.contiguous(), mask_m.contiguous()
    _lib.require_int32_masks(mc, mm)
    B, C, hh, ww = h.shape
    if tuple(hm.shape) != (B, C, hh, ww) or mc.numel() != B * (hh // 2) * (ww // 2) or mm.numel() != B * hh * ww:
        raise ValueError(refusal)
    if out is None:
        out = torch.empty_like(h)
    with _lib.on_device(h.device):
        _lib.call("cgic_decoder_blend_medium_f32", _lib.ptr(h), _lib.ptr(hm), _lib.ptr(mc), _lib.ptr(mm), B, C, hh, ww,
                  _lib.ptr(out), _lib.current_stream(h.device))
    return out


def decoder_blend_fine(h, h_fine, mask_c, mask_m, mask_f, out=None):
    """h * up4(mask_c) + h * up2(mask_m) + h_fine * mask_f on the fine grid (decoder.py:375-378) -> `out` (in place if `out is h`),
    or a new tensor"""
    _lib.require_device(h, h_fine, mask_c, mask_m, mask_f)
    h, hf = h.contiguous().float(), h_fine.contiguous().float()
    mc, mm, mf = (m.contiguous() for m in (mask_c, mask_m, mask_f))
    _lib.require_int32_masks(mc, mm, mf)
    B, C, hh, ww = h.shape
    if tuple(hf.shape) != (B, C, hh, ww) or mc.numel() != B * (hh // 4) * (ww // 4) or mm.numel() != B * (hh // 2) * (ww // 2) \
            or mf.numel() != B * hh * ww:
        raise ValueError("decoder_blend_fine: h, h_fine on the fine grid; masks at 1/4, 1/2, 1/1 of it")
    if out is None:
        out = torch.empty_like(h)
    with _lib.on_device(h.device):
        _lib.call("cgic_decoder_blend_fine_f32", _lib.ptr(h), _lib.ptr(hf), _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf), B, C, hh, ww,
                  _lib.ptr(out), _lib.current_stream(h.device))
    return out
