"""`torch.ops.cgic.*` -- the hot-path kernels as PyTorch custom ops (torch.library), so that they carry a schema, shape
inference under FakeTensor / torch.compile, and (for the quantiser) an autograd formula.  The implementations are one-line calls of the
functions the module classes use (each entry point of libcgic_hip.so is bound once, in the module that owns it: DESIGN.md); CPU tensors raise (there is no CPU fallback).

    z_q, loss, idx = torch.ops.cgic.vq_forward(z, codebook, 0.25, True)
    e8, e16        = torch.ops.cgic.entropy_maps(x)
    mc, mm, mf     = torch.ops.cgic.router(e16, e8, 0.1, 0.8, True)
    data, nbytes   = torch.ops.cgic.compress_streams(idx, mc, mm, mf, mode, table, None)          # table = HuffmanCoding(...).table.handle.value
    ind, dc, dm, df, z_q, status = torch.ops.cgic.decompress_streams(data, nbytes, h, w, mode, table, codebook, "auto")
    h = torch.ops.cgic.grain_merge(h_c, h_m, h_f, mc, mm, mf)                                     # differentiable (vqvae_blocks.py:361-366)
    nbytes = torch.ops.cgic.rate_table(ind_c, ind_m, ind_f, e16, e8, [0.1, 0.2], [0.8, 0.5], True, table)   # [C,B,5] bytes per ratio
    nbytes = torch.ops.cgic.rate_curve(ind_c, ind_m, ind_f, e16, e8, 0.1, table)                          # [B,n8+1,5] bytes per medium rank
    mc, mm, mf, ind, choice = torch.ops.cgic.route_to_bpp(ind_c, ind_m, ind_f, e16, e8, 0.1, budget, table)  # the rank picked on the device
    ind    = torch.ops.cgic.gather_grain_indices(ind_c, ind_m, ind_f, mc, mm, mf)                 # the merged latent's indices
    rec    = torch.ops.cgic.paste_tiles([tiles_of_group0, ...], H, W, N, 768, True, False)        # decoded tiles -> [N,3,H,W] (frames: uint8 [N,H,W,3])
    pmap   = torch.ops.cgic.partition_map(x, mc, mm, mf, False)                                   # the grain grid drawn into the batch (draw.py:78-119)
    blob, total = torch.ops.cgic.container_pack(data, nbytes, mode, 256, 256, 0)                  # the batch as a container file, on the device
    new_f  = torch.ops.cgic.spatial_norm(f, zq, gn_w, gn_b, wy, by, wb, bb, 32, 1e-6, False, False) # the decoder's SpatialNorm (decoder.py:34-53); defined in norm.py, next to its module
    h      = torch.ops.cgic.group_norm(f, gn_w, gn_b, 32, 1e-6, True, False)                      # the encoder's GroupNorm (+ swish) on the same kernels without zq; norm.py (group_norm_train: differentiable)
    h_     = torch.ops.cgic.attention(q, k, v, int(C) ** -0.5, False)                            # AttnBlock's softmax(q^T k) v without the [B,N,N] matrix; defined in attention.py, next to its module
    h_, lse = torch.ops.cgic.attention_train(q, k, v, int(C) ** -0.5)                             # the same, differentiable: its backward is csrc/cgic_attn_bwd.hip, no [B,N,N] matrix there either
    torch.ops.cgic.ema_update(shadows, params, decay, num_updates)                                # LitEma.forward over all tensors in one launch (ema.py:25-44), in place; defined in ema.py, next to its module
    torch.ops.cgic.adam_step(params, grads, m, v, steps, lr, b1, b2, eps, wd, clip, None, shadows, decay, num_updates)   # clip by value + Adam's step + LitEma over all tensors in one pass, in place; defined in adam.py, next to its class

A code table travels through an op as an integer: the `cgic_table*` handle of include/cgic_hip.h (ops take tensors and
scalars; the table is host-side state of the library, built once per frequency table).
"""
import ctypes
from typing import List, Optional, Tuple

import torch

from . import _lib, codec as _codec, indices_coding as _coding, merge as _merge, quantize as _quantize
from . import ema as _ema                    # noqa: F401  (registers torch.ops.cgic.ema_update)
from . import adam as _adam                  # noqa: F401  (registers torch.ops.cgic.adam_step)
from .entropy import entropy_maps as _entropy_maps, entropy_maps_u8 as _entropy_maps_u8
from .quantize import _vq_forward, vq_backward as _vq_backward, vq_forward_route as _vq_forward_route
from .router import TripleGrainFixedEntropyRouter

_DEV = "cuda"


@torch.library.custom_op("cgic::vq_forward", mutates_args=(), device_types=_DEV)
def vq_forward(z: torch.Tensor, codebook: torch.Tensor, beta: float, legacy: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """VectorQuantize2.forward (quantize.py:69-97): (z_q [B,C,h,w], loss [], indices [B*h*w] int64)"""
    z_q, loss, idx = _vq_forward(z, codebook, beta, legacy, None)
    return z_q, loss, idx


@vq_forward.register_fake
def _(z, codebook, beta, legacy):
    B, C, h, w = z.shape
    return z.new_empty(z.shape), z.new_empty(()), z.new_empty((B * h * w,), dtype=torch.int64)


@torch.library.custom_op("cgic::vq_backward", mutates_args=(), device_types=_DEV)
def vq_backward(z: torch.Tensor, codebook: torch.Tensor, indices: torch.Tensor, g_zq: torch.Tensor, g_loss: torch.Tensor,
                beta: float, legacy: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """gradients of (z_q, loss) w.r.t. (z, codebook) -- quantize.py:85-93 under autograd; deterministic"""
    gz, gw = _vq_backward(z, codebook, indices, g_zq, g_loss, beta, legacy)
    return gz, gw


@vq_backward.register_fake
def _(z, codebook, indices, g_zq, g_loss, beta, legacy):
    return z.new_empty(z.shape), codebook.new_empty(codebook.shape)


def _vq_setup(ctx, inputs, output):
    z, codebook, beta, legacy = inputs
    ctx.save_for_backward(z, codebook, output[2])
    ctx.beta, ctx.legacy = beta, legacy


def _vq_bwd(ctx, g_zq, g_loss, _g_idx):
    z, codebook, idx = ctx.saved_tensors
    if g_zq is None:
        g_zq = torch.zeros_like(z)
    if g_loss is None:
        g_loss = torch.zeros((), dtype=torch.float32, device=z.device)
    gz, gw = torch.ops.cgic.vq_backward(z, codebook, idx, g_zq, g_loss, ctx.beta, ctx.legacy)
    return gz, gw, None, None


vq_forward.register_autograd(_vq_bwd, setup_context=_vq_setup)


@torch.library.custom_op("cgic::entropy_maps", mutates_args=(), device_types=_DEV)
def entropy_maps(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Entropy(8)(x), Entropy(16)(x) in one pass (model.py:100-101,433-483): ([B,H/8,W/8], [B,H/16,W/16])"""
    e8, e16 = _entropy_maps(x)
    return e8, e16


@entropy_maps.register_fake
def _(x):
    B, _, H, W = x.shape
    return x.new_empty((B, H // 8, W // 8)), x.new_empty((B, H // 16, W // 16))


@torch.library.custom_op("cgic::entropy_maps_reference_order", mutates_args=(), device_types=_DEV)
def entropy_maps_reference_order(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """entropy_maps in the reference's own arithmetic (cgic_entropy_maps_ref_f32): torch's CPU summation order, exp / log
    correctly rounded -- the masks of tie-heavy content then agree with the CPU reference's"""
    e8, e16 = _entropy_maps(x, reference_order=True)
    return e8, e16


@entropy_maps_reference_order.register_fake
def _(x):
    B, _, H, W = x.shape
    return x.new_empty((B, H // 8, W // 8)), x.new_empty((B, H // 16, W // 16))


@torch.library.custom_op("cgic::entropy_maps_u8", mutates_args=(), device_types=_DEV)
def entropy_maps_u8(frames: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """T.ToTensor() and both Entropy maps of uint8 [B,H,W,3] frames in one pass (inference.py:50-59 + model.py:99-101):
    (x [B,3,H,W] fp32, e8, e16)"""
    x, e8, e16 = _entropy_maps_u8(frames)
    return x, e8, e16


@entropy_maps_u8.register_fake
def _(frames):
    B, H, W, _ = frames.shape
    f = lambda *s: frames.new_empty(s, dtype=torch.float32)
    return f(B, 3, H, W), f(B, H // 8, W // 8), f(B, H // 16, W // 16)


@torch.library.custom_op("cgic::router", mutates_args=(), device_types=_DEV)
def router(e16: torch.Tensor, e8: torch.Tensor, coarse_ratio: float, medium_ratio: float, per_image: bool,
           pixels: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """TripleGrainFixedEntropyRouter.forward masks (RouterTriple.py:15-95): int32 [B,1,h16,w16], [B,1,2h16,2w16], [B,1,4h16,4w16];
    the mode is a function of the ratios alone: control_gic_amd.TripleGrainFixedEntropyRouter(c, m).mode.
    pixels: the image batch behind the maps -> threshold-band refinement (masks equal to the CPU reference's from pixels)"""
    mask, _, _, _ = TripleGrainFixedEntropyRouter(coarse_ratio, medium_ratio, per_image=per_image)(e16, e8, want_gate=False, pixels=pixels)
    return mask[0], mask[1], mask[2]


@router.register_fake
def _(e16, e8, coarse_ratio, medium_ratio, per_image, pixels=None):
    B, h16, w16 = e16.shape
    mk = lambda s: e16.new_empty((B, 1, s * h16, s * w16), dtype=torch.int32)
    return mk(1), mk(2), mk(4)


@torch.library.custom_op("cgic::vq_forward_route", mutates_args=(), device_types=_DEV)
def vq_forward_route(z: torch.Tensor, codebook: torch.Tensor, beta: float, legacy: bool, e16: torch.Tensor, e8: torch.Tensor,
                     coarse_ratio: float, medium_ratio: float, per_image: bool,
                     pixels: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """vq_forward and router in ONE launch: (z_q, loss, indices, mask_c, mask_m, mask_f); pixels: see router"""
    z_q, loss, idx, mask, _, _ = _vq_forward_route(z, codebook, beta, legacy, e16, e8, coarse_ratio, medium_ratio, per_image=per_image,
                                                   pixels=pixels)
    return z_q, loss, idx, mask[0], mask[1], mask[2]


@vq_forward_route.register_fake
def _(z, codebook, beta, legacy, e16, e8, coarse_ratio, medium_ratio, per_image, pixels=None):
    B, C, h, w = z.shape
    _, h16, w16 = e16.shape
    mk = lambda s: e16.new_empty((B, 1, s * h16, s * w16), dtype=torch.int32)
    return z.new_empty(z.shape), z.new_empty(()), z.new_empty((B * h * w,), dtype=torch.int64), mk(1), mk(2), mk(4)


@torch.library.custom_op("cgic::gather_grain_indices", mutates_args=(), device_types=_DEV)
def gather_grain_indices(ind_c: torch.Tensor, ind_m: torch.Tensor, ind_f: torch.Tensor, mask_c: torch.Tensor, mask_m: torch.Tensor,
                         mask_f: torch.Tensor) -> torch.Tensor:
    """the merged latent's VQ indices from the per-head ones (include/cgic_hip.h section I): int64 [B,h,w] =
    mask_f ? ind_f : up2(mask_m) ? up2(ind_m) : up4(ind_c)"""
    from .rate import gather_grain_indices as _gather
    return _gather(ind_c, ind_m, ind_f, (mask_c, mask_m, mask_f))


@gather_grain_indices.register_fake
def _(ind_c, ind_m, ind_f, mask_c, mask_m, mask_f):
    return ind_f.new_empty((mask_f.shape[0], mask_f.shape[-2], mask_f.shape[-1]), dtype=torch.int64)


@torch.library.custom_op("cgic::paste_tiles", mutates_args=(), device_types=_DEV)
def paste_tiles(pixels: List[torch.Tensor], H: int, W: int, N: int, tile: int, weighted: bool, frames: bool) -> torch.Tensor:
    """the way out of the tiling driver (inference_high_resolution.py:231-255, write_images :103) in one launch: pixels = per shape
    group of the HxW image's `tile` grid (cut_groups order) fp32 [N*T,3,th,tw] -> [N,3,H,W] fp32, or uint8 frames [N,H,W,3]"""
    from .highres import paste_tiles as _paste_tiles
    return _paste_tiles([p.contiguous() for p in pixels], (H, W), N=N, weighted=weighted, frames=frames, tile=tile)


@paste_tiles.register_fake
def _(pixels, H, W, N, tile, weighted, frames):
    if frames:
        return pixels[0].new_empty((N, H, W, 3), dtype=torch.uint8)
    return pixels[0].new_empty((N, 3, H, W), dtype=torch.float32)


@torch.library.custom_op("cgic::partition_map", mutates_args=(), device_types=_DEV)
def partition_map(x: torch.Tensor, mask_c: torch.Tensor, mask_m: torch.Tensor, mask_f: torch.Tensor, frames: bool) -> torch.Tensor:
    """the partition map of a batch (CGIC/modules/draw.py:78-119 on the masks' grain indices) in one launch: x fp32 [B,3,H,W] or uint8
    frames [B,H,W,3] + the router's three int32 masks -> fp32 [B,3,H,W] (line pixels -1), or with frames the uint8 [B,H,W,3] (line pixels 1)"""
    from .draw import partition_map as _partition_map
    return _partition_map(x, (mask_c, mask_m, mask_f), frames=frames)


@partition_map.register_fake
def _(x, mask_c, mask_m, mask_f, frames):
    if x.dtype == torch.uint8:
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
    else:
        B, H, W = x.shape[0], x.shape[2], x.shape[3]
    if frames:
        return x.new_empty((B, H, W, 3), dtype=torch.uint8)
    return x.new_empty((B, 3, H, W), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------
# the codec (CGIC.compress, model.py:217-260 / :269-397) and the single-stream coders (indices_coding.py, mask_coding.py)
def _table(handle: int):
    if not handle:
        raise ValueError("cgic ops: the code table handle is NULL (pass HuffmanCoding(...).table.handle.value)")
    return ctypes.c_void_p(int(handle))


@torch.library.custom_op("cgic::compress_streams", mutates_args=("hist",), device_types=_DEV)
def compress_streams(ind: torch.Tensor, mask_c: torch.Tensor, mask_m: torch.Tensor, mask_f: torch.Tensor, mode: int, table: int,
                     hist: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """masked select + Huffman + mask packing of a batch (model.py:217-260): (data uint8 [B,5,slot], nbytes int32 [B,5];
    -1 = stream not written in this mode); `hist` (int64 [n_e]) accumulates the usage histogram of `ind` in the same launch"""
    comp = _codec.compress_streams(_table(table), ind, (mask_c, mask_m, mask_f), mode, hist)
    return comp.data, comp.nbytes


@compress_streams.register_fake
def _(ind, mask_c, mask_m, mask_f, mode, table, hist):
    B, h, w = mask_f.shape[0], mask_f.shape[-2], mask_f.shape[-1]
    return (ind.new_empty((B, _lib.NUM_STREAMS, _codec.slot_bytes(_table(table), h, w)), dtype=torch.uint8),
            ind.new_empty((B, _lib.NUM_STREAMS), dtype=torch.int32))


@torch.library.custom_op("cgic::container_pack", mutates_args=(), device_types=_DEV)
def container_pack(data: torch.Tensor, nbytes: torch.Tensor, mode: int, height: int, width: int, first_image_id: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the container of one batch of whole images (container.pack_device on one group; cgic_container_pack): data uint8 [B,5,slot] and
    nbytes int32 [B,5] as compress_streams returns them -> (blob uint8 [12 + 44 B + 5 B slot], total int64 [1]): blob[:total] ==
    container.pack(entries_from_batch(...)); total < 0: a stream of the batch failed (cgic_container_pack)"""
    from .codec import CompressedBatch
    from .container import pack_device
    _lib.require_device(data, nbytes)
    if data.dim() != 3 or data.shape[1] != _lib.NUM_STREAMS or data.dtype != torch.uint8 or nbytes.dtype != torch.int32:
        raise ValueError("container_pack: data uint8 [B,5,slot] and nbytes int32 [B,5]")
    # (the grid of the latent is not part of the file: CompressedBatch only carries it for decompress)
    p = pack_device(CompressedBatch(data.contiguous(), nbytes.contiguous(), mode, height // 4, width // 4), height, width, first_image_id)
    return p.blob, p.total


@container_pack.register_fake
def _(data, nbytes, mode, height, width, first_image_id):
    B, slot = data.shape[0], data.shape[2]
    return data.new_empty((12 + 44 * B + _lib.NUM_STREAMS * B * slot,), dtype=torch.uint8), data.new_empty((1,), dtype=torch.int64)


@torch.library.custom_op("cgic::rate_curve", mutates_args=(), device_types=_DEV)
def rate_curve(ind_c: torch.Tensor, ind_m: torch.Tensor, ind_f: torch.Tensor, e16: torch.Tensor, e8: torch.Tensor, coarse: float,
               table: int) -> torch.Tensor:
    """exact .bin sizes of EVERY medium rank K = 0 .. n8 at the coarse ratio `coarse`, per-image routing on the maps as given
    (cgic_rate_curve): int32 [B,n8+1,5], 0 = stream not written in the curve's mode"""
    from .rate import rate_curve as _rate_curve
    # (ranks=(): the op returns the sizes only; which ranks a ratio reaches is host arithmetic the caller may not want)
    return _rate_curve(_table(table), ind_c, ind_m, ind_f, e16, e8, coarse, ranks=()).nbytes


@rate_curve.register_fake
def _(ind_c, ind_m, ind_f, e16, e8, coarse, table):
    return e16.new_empty((e16.shape[0], 4 * e16.shape[1] * e16.shape[2] + 1, _lib.NUM_STREAMS), dtype=torch.int32)


@torch.library.custom_op("cgic::route_to_bpp", mutates_args=(), device_types=_DEV)
def route_to_bpp(ind_c: torch.Tensor, ind_m: torch.Tensor, ind_f: torch.Tensor, e16: torch.Tensor, e8: torch.Tensor, coarse: float,
                 budget: torch.Tensor, table: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """route the batch at the medium rank whose batch size is the largest one within `budget` bytes (int64 [1] on the device),
    decided on the device without a host synchronisation (cgic_route_to_budget): (mask_c, mask_m, mask_f int32 in the router's
    layouts, ind int64 [B,h,w], choice int64 [4] = {j, K, fits, batch bytes}; all -1, fits 0 and zero outputs when a requested
    entry holds a symbol outside the table)"""
    from .rate import route_to_bpp as _route_to_bpp
    r = _route_to_bpp(_table(table), ind_c, ind_m, ind_f, e16, e8, coarse, budget=budget)
    return r.masks[0], r.masks[1], r.masks[2], r.ind, r.choice


@route_to_bpp.register_fake
def _(ind_c, ind_m, ind_f, e16, e8, coarse, budget, table):
    B, h16, w16 = e16.shape
    return (e16.new_empty((B, 1, h16, w16), dtype=torch.int32), e16.new_empty((B, 1, 2 * h16, 2 * w16), dtype=torch.int32),
            e16.new_empty((B, 1, 4 * h16, 4 * w16), dtype=torch.int32), e16.new_empty((B, 4 * h16, 4 * w16), dtype=torch.int64),
            e16.new_empty((4,), dtype=torch.int64))


@torch.library.custom_op("cgic::rate_table", mutates_args=(), device_types=_DEV)
def rate_table(ind_c: torch.Tensor, ind_m: torch.Tensor, ind_f: torch.Tensor, e16: torch.Tensor, e8: torch.Tensor, coarse: List[float],
               medium: List[float], per_image: bool, table: int, pixels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """exact .bin sizes per candidate ratio (coarse[c], medium[c]) without writing a stream (cgic_rate_table): int32 [C,B,5],
    0 = stream not written in that mode; pixels: see router"""
    if len(coarse) != len(medium):
        raise ValueError("rate_table: one medium ratio per coarse ratio")
    from .rate import rate_table as _rate_table
    return _rate_table(_table(table), ind_c, ind_m, ind_f, e16, e8, list(zip(coarse, medium)), per_image=per_image, pixels=pixels).nbytes


@rate_table.register_fake
def _(ind_c, ind_m, ind_f, e16, e8, coarse, medium, per_image, table, pixels=None):
    return e16.new_empty((len(coarse), e16.shape[0], _lib.NUM_STREAMS), dtype=torch.int32)


@torch.library.custom_op("cgic::decompress_streams", mutates_args=(), device_types=_DEV)
def decompress_streams(data: torch.Tensor, nbytes: torch.Tensor, h: int, w: int, mode: int, table: int, codebook: torch.Tensor,
                       decoder: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """prefix decode + mask rebuild + x2/x4 merge + embedding gather (model.py:269-397):
    (ind int64 [B,h,w], mask_c, mask_m, mask_f int32 [B,1,.,.], z_q fp32 [B,4,h,w], status int32 [B]);
    decoder: "auto" / "latency" / "throughput" -- a property of this call"""
    _lib.require_device(data, nbytes, codebook)
    if decoder not in _codec.DECODERS:
        raise ValueError(f"decoder {decoder!r}: expected one of {sorted(_codec.DECODERS)}")
    comp = _codec.CompressedBatch(data.contiguous(), nbytes.contiguous(), mode, h, w)
    # (the decoder is named explicitly, "auto" included: an enclosing decoder_mode block does not reach into an op)
    ind, (mc, mm, mf), zq, status = _codec.decompress_streams(_table(table), comp, codebook, decoder=decoder)
    return ind, mc, mm, mf, zq, status


@decompress_streams.register_fake
def _(data, nbytes, h, w, mode, table, codebook, decoder):
    B = data.shape[0]
    i32 = lambda *s: data.new_empty(s, dtype=torch.int32)
    return (data.new_empty((B, h, w), dtype=torch.int64), i32(B, 1, h // 4, w // 4), i32(B, 1, h // 2, w // 2), i32(B, 1, h, w),
            codebook.new_empty((B, codebook.shape[1], h, w)), i32(B))


@torch.library.custom_op("cgic::encode_stream", mutates_args=(), device_types=_DEV)
def encode_stream(symbols: torch.Tensor, table: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """HuffmanCoding.compress / BinaryCoding.compress without the file (indices_coding.py:113-126, mask_coding.py:40-55):
    (bytes uint8 [capacity], nbytes int32 [1]); symbols: 1-D int64 / int32, at least one"""
    _lib.require_device(symbols)
    info = symbols.reshape(-1).contiguous()
    if info.dtype not in (torch.int64, torch.int32):
        raise TypeError("encode_stream: int64 / int32 symbols")
    if info.numel() == 0:
        raise ValueError("encode_stream: an empty input is an empty FILE in the reference (indices_coding.py:116-118), not a stream")
    return _coding.encode_stream(_table(table), info)


@encode_stream.register_fake
def _(symbols, table):
    cap = _coding.stream_capacity(_table(table), symbols.numel())
    return symbols.new_empty((cap,), dtype=torch.uint8), symbols.new_empty((1,), dtype=torch.int32)


@torch.library.custom_op("cgic::decode_stream", mutates_args=(), device_types=_DEV)
def decode_stream(stream: torch.Tensor, nbytes: int, table: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """HuffmanCoding.decompress_string / BinaryCoding.decompress_string without the file (indices_coding.py:153-168):
    (symbols int64 [(nbytes - 1) * 8] of which the first `count` are valid, count int64 [1]; -1 = the empty file's None).
    stream: uint8, at least nbytes + 16 readable bytes"""
    _lib.require_device(stream)
    if stream.dtype != torch.uint8 or stream.numel() < nbytes + 16:
        raise ValueError("decode_stream: uint8 buffer of at least nbytes + 16 bytes")
    return _coding.decode_stream(_table(table), stream.contiguous(), nbytes)


@decode_stream.register_fake
def _(stream, nbytes, table):
    return stream.new_empty((max(1, (nbytes - 1) * 8),), dtype=torch.int64), stream.new_empty((1,), dtype=torch.int64)


@torch.library.custom_op("cgic::index_histogram", mutates_args=("hist",), device_types=_DEV)
def index_histogram(indices: torch.Tensor, hist: torch.Tensor) -> None:
    """hist[indices[i]] += 1 (quantize.py:79-81), exact int64"""
    _quantize.index_histogram(indices, hist)


# ------------------------------------------------------------------------------------------------------------------
# the mask-merge kernels either side of the quantiser (vqvae_blocks.py:361-366, decoder.py:304-305,366-378): they sit inside the
# reference's training graph, so they carry autograd formulas.  The masks are constants of the graph (int32, from the router).
def _up(m, k):
    return m.to(torch.float32).repeat_interleave(k, dim=-2).repeat_interleave(k, dim=-1)


@torch.library.custom_op("cgic::grain_merge", mutates_args=(), device_types=_DEV)
def grain_merge(h_coarse: torch.Tensor, h_medium: torch.Tensor, h_fine: torch.Tensor, mask_c: torch.Tensor, mask_m: torch.Tensor,
                mask_f: torch.Tensor) -> torch.Tensor:
    """up4(h_coarse)*up4(mask_c) + up2(h_medium)*up2(mask_m) + h_fine*mask_f in one pass (vqvae_blocks.py:361-366), bit-identical"""
    return _merge.grain_merge(h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f)


@grain_merge.register_fake
def _(h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f):
    return h_fine.new_empty(h_fine.shape, dtype=torch.float32)


def _grain_merge_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[3:])


def _grain_merge_bwd(ctx, g):
    mc, mm, mf = ctx.saved_tensors
    g = g.contiguous()
    B, _, h, w = g.shape
    # masks arrive as [B,1,.,.] or squeezed [B,.,.] (the forward only needs their element count): broadcast over channels
    # explicitly -- a squeezed [B,h,w] mask with B == C would otherwise line up with the CHANNEL axis and scale silently wrong
    mc = mc.reshape(B, 1, h // 4, w // 4).to(g.dtype)
    mm = mm.reshape(B, 1, h // 2, w // 2).to(g.dtype)
    mf = mf.reshape(B, 1, h, w).to(g.dtype)
    # d/dh_coarse = mask_c * (sum of g over the 4x4 cell): the window sum is the library's average pool x 16 (exact)
    g_c = torch.ops.cgic.avg_pool(g, 4) * 16.0 * mc
    g_m = torch.ops.cgic.avg_pool(g, 2) * 4.0 * mm
    return g_c, g_m, g * mf, None, None, None


grain_merge.register_autograd(_grain_merge_bwd, setup_context=_grain_merge_setup)


@torch.library.custom_op("cgic::avg_pool", mutates_args=(), device_types=_DEV)
def avg_pool(x: torch.Tensor, k: int) -> torch.Tensor:
    """torch.nn.AvgPool2d(k, k, 0) for k in (2, 4) (decoder.py:304-305,366-367): row-major window sum / k^2, bit-identical to the CPU kernel;
    H and W must be multiples of k (the decoder's are; cgic_avgpool_f32 refuses anything else)"""
    return _merge.avg_pool(x, k)


@avg_pool.register_fake
def _(x, k):
    B, C, H, W = x.shape
    return x.new_empty((B, C, H // k, W // k), dtype=torch.float32)


def _avg_pool_setup(ctx, inputs, output):
    ctx.k = inputs[1]


def _avg_pool_bwd(ctx, g):
    k = ctx.k                                                            # (H and W are multiples of k: the forward refuses others)
    return (g * (1.0 / (k * k))).repeat_interleave(k, dim=-2).repeat_interleave(k, dim=-1), None


avg_pool.register_autograd(_avg_pool_bwd, setup_context=_avg_pool_setup)


@torch.library.custom_op("cgic::decoder_blend_medium", mutates_args=(), device_types=_DEV)
def decoder_blend_medium(h: torch.Tensor, h_medium: torch.Tensor, mask_c: torch.Tensor, mask_m: torch.Tensor) -> torch.Tensor:
    """h * up2(mask_c) + h_medium * mask_m on the medium grid (decoder.py:372-374)"""
    return _merge.decoder_blend_medium(h, h_medium, mask_c, mask_m,
                                       "decoder_blend_medium: h, h_medium on the medium grid; mask_c at half of it, mask_m on it")


@decoder_blend_medium.register_fake
def _(h, h_medium, mask_c, mask_m):
    return h.new_empty(h.shape, dtype=torch.float32)


def _blend_m_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[2], inputs[3])


def _blend_m_bwd(ctx, g):
    mc, mm = ctx.saved_tensors
    B = g.shape[0]
    return g * _up(mc.reshape(B, 1, g.shape[-2] // 2, g.shape[-1] // 2), 2), g * mm.reshape(B, 1, g.shape[-2], g.shape[-1]).to(g.dtype), None, None


decoder_blend_medium.register_autograd(_blend_m_bwd, setup_context=_blend_m_setup)


@torch.library.custom_op("cgic::decoder_blend_fine", mutates_args=(), device_types=_DEV)
def decoder_blend_fine(h: torch.Tensor, h_fine: torch.Tensor, mask_c: torch.Tensor, mask_m: torch.Tensor, mask_f: torch.Tensor) -> torch.Tensor:
    """h * up4(mask_c) + h * up2(mask_m) + h_fine * mask_f on the fine grid (decoder.py:375-378)"""
    return _merge.decoder_blend_fine(h, h_fine, mask_c, mask_m, mask_f)


@decoder_blend_fine.register_fake
def _(h, h_fine, mask_c, mask_m, mask_f):
    return h.new_empty(h.shape, dtype=torch.float32)


def _blend_f_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[2:])


def _blend_f_bwd(ctx, g):
    mc, mm, mf = ctx.saved_tensors
    B, _, hh, ww = g.shape
    # (the reference's expression adds h twice where both coarser masks are set; they never overlap in a router's output)
    wh = _up(mc.reshape(B, 1, hh // 4, ww // 4), 4) + _up(mm.reshape(B, 1, hh // 2, ww // 2), 2)
    return g * wh, g * mf.reshape(B, 1, hh, ww).to(g.dtype), None, None, None


decoder_blend_fine.register_autograd(_blend_f_bwd, setup_context=_blend_f_setup)
