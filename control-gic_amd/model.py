"""Drop-in for the hot-path parts of the CGIC LightningModule (CGIC/models/model.py).

`install(model)` swaps the hot-path submodules of an existing reference `CGIC` instance for the MI355X
ones in place (same state_dict keys, so the published checkpoint keeps loading) and rebinds
`model.compress`.  `compress` keeps the reference's signature and return value; `compress_batch` is the
batched form the reference does not have (its `compress` raises IndexError for B > 1, model.py:219).
The conv encoder / decoder stay whatever the model already has (stock PyTorch; out of scope here).
"""
import types

import torch

from . import draw as _draw
from . import adam as _adam
from . import ema as _ema
from . import merge as _merge
from . import norm as _norm
from .attention import patch_attention as _patch_attention      # (the package exports the FUNCTION attention under the module's name)
from . import rate as _rate
from . import resblock as _resblock
from .codec import GrainCodec
from .entropy import Entropy
from .indices_coding import HuffmanCoding
from .quantize import FusedQuantConv, VectorQuantize2
from .router import routing_per_image

ROUTER_TARGET = "control_gic_amd.router.TripleGrainFixedEntropyRouter"


def _raw(*feats):
    """no autograd is needed for these features: the raw kernel call may serve them"""
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in feats))


def grain_merge(h_coarse, h_medium, h_fine, mask, out_dtype=None):
    """h = up4(h_coarse)*up4(mask[0]) + up2(h_medium)*up2(mask[1]) + h_fine*mask[2]
    (vqvae_blocks.py:361-366) in one pass; mask = the router's three int32 tensors.  Differentiable w.r.t. the three
    latents (torch.ops.cgic.grain_merge: the op sits inside the reference's training graph).  The result is fp32 like the
    reference's expression, also for fp16 / bf16 latents; out_dtype = their half type (the raw kernel call, no autograd) rounds it
    once to that type."""
    if out_dtype is None:
        return torch.ops.cgic.grain_merge(h_coarse, h_medium, h_fine, mask[0], mask[1], mask[2])
    return _merge.grain_merge(h_coarse, h_medium, h_fine, mask[0], mask[1], mask[2], out_dtype=out_dtype)


def avg_pool(x, k):
    """torch.nn.AvgPool2d(k, k, 0) for k in (2, 4) -- decoder.py:304-305,366-367; bit-identical to the CPU kernel
    (row-major running sum of the window, divided by k*k); differentiable (torch.ops.cgic.avg_pool)"""
    return torch.ops.cgic.avg_pool(x, int(k))


def decoder_blend_medium(h, h_medium, mask, out=None, out_dtype=None):
    """h * up2(mask[0]) + h_medium * mask[1] on the medium grid (decoder.py:372-374).  Differentiable
    (torch.ops.cgic.decoder_blend_medium); with `out` (which may be `h`: in place) or `out_dtype` the raw kernel call, no
    autograd.  fp32 out, also for fp16 / bf16 features (the reference's promotion), unless `out` / `out_dtype` is their half type."""
    if out is None and out_dtype is None:
        return torch.ops.cgic.decoder_blend_medium(h, h_medium, mask[0], mask[1])
    return _merge.decoder_blend_medium(h, h_medium, mask[0], mask[1],
                                       "decoder_blend_medium: h, h_medium on the medium grid; mask[0] at half of it, mask[1] on it", out=out,
                                       out_dtype=out_dtype)


def decoder_blend_fine(h, h_fine, mask, out=None, out_dtype=None):
    """h * up4(mask[0]) + h * up2(mask[1]) + h_fine * mask[2] on the fine grid (decoder.py:375-378).  Differentiable
    (torch.ops.cgic.decoder_blend_fine); with `out` (in place if `out is h`) or `out_dtype` the raw kernel call, no autograd.
    fp32 out, also for fp16 / bf16 features (the reference's promotion), unless `out` / `out_dtype` is their half type."""
    if out is None and out_dtype is None:
        return torch.ops.cgic.decoder_blend_fine(h, h_fine, mask[0], mask[1], mask[2])
    return _merge.decoder_blend_fine(h, h_fine, *mask, out=out, out_dtype=out_dtype)


def _codec_for(model, h_indices=None):
    """the model's GrainCodec, rebuilt when what it was built from changed: the codebook tensor, the usage counters (the
    Huffman table IS the counters: a train() step between two compress() calls changes it -- round 3 kept a stale table), or the
    coder object the caller hands in.  `h_indices` (model.py:206): a control_gic_amd HuffmanCoding is used as it is; a FOREIGN
    coder (the reference's own class, whose codes the GPU coder cannot take over) must describe the same code as the counters
    do, otherwise its files would not be what this compress() writes: that raises instead of being ignored."""
    q = model.quantize
    own = h_indices if isinstance(h_indices, HuffmanCoding) else None
    counter = q.usage_counter if hasattr(q, "usage_counter") else None
    c = getattr(model, "_cgic_codec", None)
    key = getattr(model, "_cgic_codec_key", None)
    fresh = (c is not None and key is not None and c.codebook is q.embedding.weight and key[0] is own
             and (counter is None or (key[1].device == counter.device and torch.equal(key[1], counter))))
    if not fresh:
        huff = own if own is not None else HuffmanCoding(q.embedding_counter)
        c = GrainCodec(huff, q.embedding.weight)
        model._cgic_codec = c
        model._cgic_codec_key = (own, None if counter is None else counter.detach().clone())
    if h_indices is not None and own is None:
        theirs = getattr(h_indices, "codes", None)
        if not isinstance(theirs, dict) or {int(k): v for k, v in theirs.items()} != c.huffman.codes:
            raise ValueError("compress(h_indices=...): the coder handed in does not carry the code table of this model's "
                             "embedding_counter (or is not a Huffman coder with .codes); build it from "
                             "model.quantize.embedding_counter like inference.py:150, or pass a control_gic_amd.HuffmanCoding")
    return c


def compress_batch(model, input, h_indices=None, decode=True, save_img=False):
    """batched CGIC.compress (model.py:206-401): -> (dec [B,3,H,W] or None, bpp list[B], CompressedBatch).
    Every image is routed on its own thresholds (what B independent B=1 calls of the reference give).
    save_img: the returned CompressedBatch carries `.partition_map`, fp32 [B,3,H,W]: the input with the grain grid of the routing
    that was used drawn in as -1 (draw.partition_map on the masks: one launch; model.py:213-214)."""
    assert len(input.shape) == 4                                         # model.py:207
    codec = _codec_for(model, h_indices)
    # "B independent B=1 calls": every image routed on its own thresholds, whatever the router's batch semantics
    # for encode()/forward() are (the reference flattens the batch, RouterTriple.py:21-31)
    rc = getattr(model.encoder, "router_config", None)
    params = rc.get("params") if isinstance(rc, dict) or hasattr(rc, "get") else None
    with routing_per_image(params):
        quant, diff, grain_indices, grain_mask, ind, _, mode = model.encode(input)
    comp = codec.compress(ind, grain_mask, mode)
    bpp = comp.bpp(input.shape[2] * input.shape[3])                      # model.py:223,233
    dec = _decode(model, codec, comp) if decode else None
    if save_img:
        comp.partition_map = _draw.partition_map(input.float(), grain_mask)
    return dec, bpp, comp


def _decode(model, codec, comp):
    """the decode half of compress (model.py:269-401): streams -> indices, masks, quant -> the model's decoder"""
    pqc = getattr(model, "post_quant_conv", None)
    fuse = (getattr(model, "_cgic_fuse_post_quant_conv", False) and isinstance(pqc, torch.nn.Conv2d)
            and tuple(pqc.weight.shape) == (4, 4, 1, 1) and hasattr(model, "decoder"))
    ind_d, mask_d, quant_d, status = codec.decompress(comp, post_quant_conv=pqc if fuse else None)
    if int(status.abs().max()) != 0:
        raise RuntimeError("decoded symbol count does not match its mask")   # shape mismatch in the reference
    if fuse:
        quant, quant2 = quant_d                                          # post_quant_conv came out of the gather
        return model.decoder(quant2, quant, mask_d)                      # model.py:115-116
    return model.decode(quant_d, mask_d)                                 # model.py:399


def compress(self, input, path, h_indices=None, h_mask=None, save_img=False):
    """CGIC.compress with the reference's signature and return value (dec, bpp, partition_map); also
    leaves the reference's five .bin files for the image in `path` (model.py:226-249).  B must be 1 like
    the reference; use compress_batch for more.
    save_img=True: partition_map = fp32 [1,3,H,W], the input with the grain grid drawn in as -1 (model.py:213-214), None otherwise.
    Deliberate deviation: the map shows the routing that was USED -- draw.partition_map on the router's masks, bit-identical to the
    reference's draw_triple_grain_256res on the masks' grain indices (draw.grain_map).  The stock encoder's own `grain_indices` is
    a malformed [B,1,h] tensor (the permute at vqvae_blocks.py:357 puts the wrong axis under the argmax), whose picture is a few
    meaningless lines; draw.draw_triple_grain_256res(input.clone(), grain_indices) reproduces that picture bit for bit."""
    if input.shape[0] != 1:
        raise IndexError("compress() takes one image like the reference (model.py:219); use compress_batch")
    dec, bpp, comp = compress_batch(self, input, h_indices, save_img=bool(save_img))
    comp.write_legacy(path, 0)
    return dec, bpp[0], comp.partition_map if save_img else None


class AvgPool(torch.nn.Module):
    """torch.nn.AvgPool2d(k, k, 0) on the library's kernel (decoder.py:304-305): bit-identical to the CPU kernel, differentiable.
    A fp16 / bf16 input keeps its type like AvgPool2d's (the fp32 window sum / k^2 rounded once: the CPU kernel's value) on the half
    kernel when no autograd is needed, and takes torch's own pool when it is"""

    def __init__(self, k):
        super().__init__()
        self.k = int(k)

    def forward(self, x):
        if not x.is_cuda or x.dim() != 4 or x.shape[2] % self.k or x.shape[3] % self.k:
            return torch.nn.functional.avg_pool2d(x, self.k, self.k, 0)
        if x.dtype == torch.float32:
            return torch.ops.cgic.avg_pool(x, self.k)
        # fp16 / bf16 (the decoder under torch.autocast): AvgPool2d keeps the type; the half kernel has no autograd formula
        if x.dtype in (torch.float16, torch.bfloat16) and _raw(x):
            return _merge.avg_pool(x, self.k, out_dtype=x.dtype)
        return torch.nn.functional.avg_pool2d(x, self.k, self.k, 0)


def install(model, per_image=False, fuse_convs=True, patch_pools=True, patch_norms=False, patch_attention=False, norm_backward=False,
            attention_backward=False, patch_group_norms=False, patch_resblocks=False, patch_ema=False, patch_optimizers=False, clip_value=None):
    """swap VectorQuantize2 / Entropy / router target / compress of a reference CGIC instance in place.
    patch_pools: the decoder's two average pools in front of its masked blends (decoder.avgpool_layer1 / _layer2,
    decoder.py:304-305,366-367) become control_gic_amd.model.AvgPool -- they are modules, so they can be swapped.  The three
    masked-blend EXPRESSIONS (vqvae_blocks.py:364-366, decoder.py:372-378) are inline arithmetic of the reference's forward
    methods: using grain_merge / decoder_blend_medium / decoder_blend_fine there takes the two source edits INTEGRATION.md shows.
    per_image=False keeps the reference's routing for encode() / forward() / training (thresholds over the flattened
    batch, RouterTriple.py:21-31); compress_batch / compress / the tiling driver always route per image.
    fuse_convs: move quant_conv into the VQ kernel and post_quant_conv into the decode-side gather (under no_grad).  The
    hand-off is explicit: under no_grad `model.quant_conv(h)` returns a quantize.PendingQuantConv (its input, tagged) that
    `model.quantize` convolves inside its kernel; used anywhere else it behaves as the convolved latent, and a latent that
    reaches `model.quantize` as an ordinary tensor is quantised as it is.
    patch_norms: every module with the shape of the reference's SpatialNorm (decoder.py:34-53: norm_layer, 1x1 conv_y / conv_b,
    add_conv) becomes control_gic_amd.norm.SpatialNorm on the same parameters (csrc/cgic_norm.hip under no_grad; torch's expression
    when a gradient is needed -- or, with norm_backward=True, the library's training forward and backward kernels there too:
    SpatialNorm.backward_kernel, one kernel family forward and backward that keeps only f and two floats per group.  Forward +
    backward of the norm alone, measured over the decoder's shapes at B = 8 and 1, fp32 and autocast-fp16, one layer and a stack of
    eight: 1.1x to 4.5x faster than torch's path and 2.5x to 8.4x less peak memory, no shape slower; profiles/spatial_norm_backward.md).  Off by default, unlike patch_pools: the pools are bit-identical to torch, a normalisation agrees
    with torch's only within rounding, and the default install() keeps producing exactly what it produced before.
    patch_attention: every module with the shape of the reference's AttnBlock (decoder.py:161-213, vqvae_blocks.py:140-192:
    in_channels, norm, 1x1 q / k / v / proj_out) becomes control_gic_amd.attention.AttnBlock on the same parameters: under no_grad
    its softmax(q^T k) v runs in csrc/cgic_attn.hip and no [B,N,N] matrix is written; torch's expression when a gradient is needed
    or the width is not built.  Off by default for the reason patch_norms is.  With patch_norms as well, the block's norm is the
    fused SpatialNorm.
    attention_backward (with patch_attention): AttnBlock.backward_kernel -- an attention that needs a gradient runs the same forward
    kernel and, in the backward pass, csrc/cgic_attn_bwd.hip, so that training keeps q, k, v, out and one float per token in place of
    torch's [B,N,N] softmax and its half copy.  Forward + backward of the attention alone, measured: at [2,512,4096] in bf16 a peak
    of 32 MiB against 720 MiB for 3.5x the time (3.31 ms against 0.94 ms), at the 36 864 tokens of a 768x768 tile 144 MiB against
    28 GiB for 2.7x the time; fp32 3x to 90x less memory for 8x the time; no shape is faster (profiles/attention_backward.md).  Off by
    default, also where patch_attention is on: the gradients agree with torch's only within rounding, and the switch buys memory,
    not time -- set it where the attention blocks' activations limit the batch or the tile.  Without patch_attention there is no
    block to set it on and the call raises (norm_backward without patch_norms is ignored, as it always was: that behaviour is kept).
    patch_group_norms: every affine torch.nn.GroupNorm that is not the norm_layer of a SpatialNorm-shaped module -- the encoder's
    Normalize (vqvae_blocks.py:34) in its ResnetBlocks, AttnBlocks and norm_out heads -- becomes control_gic_amd.norm.GroupNorm, a
    subclass on the same parameters: the same kernel family without zq under no_grad, F.group_norm when a gradient is needed or, with
    norm_backward=True, the library's training forward and backward kernels (GroupNorm.backward_kernel on the norms swapped in here).
    patch_resblocks: every module with the shape of the reference's ResnetBlock (vqvae_blocks.py:78-137, decoder.py:99-158: norm1,
    conv1, norm2, dropout, conv2, in_channels, out_channels, use_conv_shortcut) becomes control_gic_amd.resblock.ResnetBlock on the
    same submodules, which passes swish=True to its norms where they are the library's (patch_group_norms / patch_norms) so that the
    swish runs inside the norm kernel, and under autocast takes the half type straight from the kernel.  The encoder's three
    norm_out + nonlinearity pairs are inline in Encoder.forward: INTEGRATION.md section 3f shows the one-line edit.  Both are off by
    default for the reason patch_norms is, and install() with neither produces exactly the module tree it produced before.  Measured
    against torch's group_norm + swish over the encoder's shapes at B = 8 and 1 (profiles/group_norm.md): 2.6x to 7.3x faster at the
    256x256 and 128x128 levels, forward and forward + backward, with 2x to 6.4x less peak memory.  SLOWER than torch's path where the
    features are small, beyond the run-to-run spread: forward in fp32 at [8,512,16,16] (0.84x) and at B = 1 from 64x64 down (0.70x to
    0.85x); forward + backward of a single layer at B = 8 from 64x64 down and at B = 1 from 128x128 down (0.58x to 0.88x) -- a call of
    the kernel route costs about 0.03 ms forward and 0.10 to 0.14 ms forward + backward in Python and launches, torch's two small
    kernels 0.02 to 0.03 ms.  Under autocast the forward is never slower.
    patch_ema: every direct attribute of the model with the shape of the reference's LitEma (ema.py:5-23: m_name2s_name, the buffers
    decay and num_updates) -- ema_encoder, ema_decoder, ema_quantize, ema_quant_conv, ema_post_quant_conv (model.py:61-66) -- becomes
    control_gic_amd.LitEma.adopt(it) on the same buffer objects: its update after every optimiser step is a one-thread launch and one
    launch over all tensors (csrc/cgic_ema.hip), bit-identical to the reference's three torch operations per tensor, with no read of
    num_updates on the host.  Names are matched against the module forward() is called with, as in the reference, so ema_quantize
    keeps working with the VectorQuantize2 swapped in above (its usage counters are not trainable and stay out).  Off by default:
    install() without it leaves the five attributes alone.  Measured on the 655 trainable tensors of the training config (130.36 M
    elements; profiles/ema.md): a step of the five modules takes 0.840 ms against 8.259 ms for the reference's per-tensor loop and
    1.289 ms for torch._foreach_* (9.83x and 1.53x), with 10 launches against 1975 and 50, no temporary against 18 MiB and 499 MiB and no
    host synchronisation against five; 0.33 ms of the 0.840 ms are kernel time (the update kernel moves its 12 B/element at 4.99 TB/s),
    the rest is the Python of forward.  copy_to, store and restore: 3.1x, 1.5x and 3.1x faster than the reference's loops.  No training step was measured.
    patch_optimizers: model.configure_optimizers is wrapped so that every optimiser it returns of EXACTLY type torch.optim.Adam becomes
    a control_gic_amd.Adam on the same param groups and defaults (adam.py; csrc/cgic_adam.hip): per param group one pass over gradient,
    parameter, exp_avg and exp_avg_sq with torch's single-tensor arithmetic, one fp32 rounding per operation; parameters the kernel
    does not take are stepped by torch's own implementation.  clip_value (with patch_optimizers): clip every gradient to +-clip_value
    inside the same pass -- leave the trainer's gradient_clip_val unset then, or the gradients are clipped twice (harmless, wasted
    work); the fused clip does not write the clipped gradients back, Lightning's does.  With patch_ema as well, the model's LitEma
    children are attached to the optimiser that owns their parameters (Adam.attach_ema): their shadows are updated inside the step and
    the reference's on_train_batch_end stays as it is.  Both off by default.  Measured on the same 655 tensors with clip 1.0 and the
    EMA on (profiles/adam.md): one optimiser tail takes 1.170 ms against 14.44 ms for clip_grad_value_ + torch.optim.Adam + the
    reference's EMA loop and 2.752 ms for clip_grad_value_ + Adam(fused=True) + cg.LitEma; the pass moves its 36 B per element at 4.96
    TB/s.  No training step was measured."""
    old = model.quantize
    dev = old.embedding.weight.device
    q = VectorQuantize2(old.n_e, old.e_dim, beta=old.beta, legacy=getattr(old, "legacy", True))
    q.load_state_dict(old.state_dict(), strict=False)
    q.to(dev).train(old.training)
    model.quantize = q
    for name, p in (("entropy_calculation_p8", 8), ("entropy_calculation_p16", 16)):
        if hasattr(model, name):
            setattr(model, name, Entropy(p))
    rc = getattr(model.encoder, "router_config", None)
    if rc is not None:
        rc["target"] = ROUTER_TARGET
        rc["params"]["per_image"] = bool(per_image)
    # the two 1x1 convolutions either side of the quantiser (model.py:51-52): quant_conv runs inside the VQ kernel,
    # post_quant_conv becomes a second gather table of the decode-side merge kernel (inference only; autograd sees Conv2d)
    if fuse_convs and isinstance(getattr(model, "quant_conv", None), torch.nn.Conv2d) \
            and tuple(model.quant_conv.weight.shape) == (4, 4, 1, 1) and q.n_e % 64 == 0 and q.n_e <= 1024:
        model.quant_conv = FusedQuantConv.adopt(model.quant_conv)          # hands its input to the quantiser as a PendingQuantConv
    model._cgic_fuse_post_quant_conv = bool(fuse_convs)
    dec = getattr(model, "decoder", None)
    if patch_pools and dec is not None:
        for name, k in (("avgpool_layer1", 4), ("avgpool_layer2", 2)):
            m = getattr(dec, name, None)
            if isinstance(m, torch.nn.AvgPool2d) and m.kernel_size in (k, (k, k)) and m.stride in (k, (k, k)) and m.padding in (0, (0, 0)):
                setattr(dec, name, AvgPool(k))
    if patch_attention:
        _patch_attention(model, backward_kernel=attention_backward)
    elif attention_backward:
        raise ValueError("install: attention_backward=True sets AttnBlock.backward_kernel on the blocks that patch_attention=True swaps in; without it there are none")
    if patch_norms:
        _norm.patch_norms(model, backward_kernel=norm_backward)
    if patch_group_norms:
        _norm.patch_group_norms(model, backward_kernel=norm_backward)
    if patch_resblocks:
        _resblock.patch_resblocks(model)
    if patch_ema:
        _ema.patch_ema(model)
    if patch_optimizers:
        _adam.patch_optimizers(model, clip_value=clip_value, attach_emas=bool(patch_ema))
    elif clip_value is not None:
        raise ValueError("install: clip_value is the clip of the cg.Adam that patch_optimizers=True swaps in; without it there is none")
    model.compress = types.MethodType(compress, model)
    model.compress_batch = types.MethodType(compress_batch, model)
    model.compress_to_bpp = types.MethodType(_rate.compress_to_bpp, model)
    model.compress_tiled_to_bpp = types.MethodType(_rate.compress_tiled_to_bpp, model)
    from . import highres as _highres
    model.to_frames = _highres.to_frames                 # the way out: inference.py:163 + write_images (:103) as one launch
    model.paste_tiles = _highres.paste_tiles             # ... and the tiled one (inference_high_resolution.py:231-255)
    model.partition_map = _draw.partition_map             # the grain grid of a batch (CGIC/modules/draw.py:78-119) as one launch
    model.partition_tiles = _highres.partition_tiles      # ... and of tiled images (what inference_high_resolution.py -w promises)
    model._cgic_codec = None
    model._cgic_codec_key = None
    return model
