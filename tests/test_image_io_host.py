"""CPU: pipeline.image_io_buffers, the one place that allocates the buffer set of a cgic_compress_image call and fills the
struct cgic_image_io that HotCall and TiledCall hand to the library.  A pointer left NULL or pointing at the wrong buffer there
is a GPU fault; here the same function runs on CPU tensors, and every field is checked against a formula written down by hand.
The expected NULL pattern is what HotCall.__init__ / TiledCall.__init__ set field by field before they shared this function:
HotCall = (x_out: u8 input, want_zq, want_loss, hist as given), TiledCall = (x_out: always, no z_q, no loss, no hist)."""
import itertools

import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib
from control_gic_amd.pipeline import image_io_buffers

B, H, W = 2, 64, 96
h, w = H // 4, W // 4
SLOT = 1000
FIELDS = [name for name, _ in _lib.ImageIO._fields_]


def expected_bytes(hist, ws_refine):
    """field -> the bytes of the buffer it must point at (hand-written from include/cgic_hip.h's description of each field)"""
    l = _lib.lib()
    return {
        "x_out": B * 3 * H * W * 4,
        "e8": B * (H // 8) * (W // 8) * 4, "e16": B * (H // 16) * (W // 16) * 4, "flat8": B * (H // 8) * (W // 8) * 4,
        "ind": B * h * w * 8, "z_q": B * 4 * h * w * 4, "loss": 4,
        "mask_c": B * (h // 4) * (w // 4) * 4, "mask_m": B * (h // 2) * (w // 2) * 4, "mask_f": B * h * w * 4,
        "streams": B * 5 * SLOT, "nbytes": B * 5 * 4, "hist": None if hist is None else hist.numel() * 8,
        "dind": B * h * w * 8, "dmask_c": B * (h // 4) * (w // 4) * 4, "dmask_m": B * (h // 2) * (w // 2) * 4, "dmask_f": B * h * w * 4,
        "dz_q": B * 4 * h * w * 4, "status": B * 4,
        "ws_vq": l.cgic_vq_workspace_bytes(B * h * w), "ws_compress": max(1, l.cgic_compress_workspace_bytes(B, h, w)),
        "ws_decompress": l.cgic_decompress_workspace_bytes(B, h, w),
        "ws_refine": None if ws_refine is None else ws_refine.numel(),
    }


def expected_null(decode, x_out, want_zq, want_loss, hist, ws_refine):
    null = {"x", "z"}                                   # the caller's, per call
    if not x_out:
        null.add("x_out")
    if not want_zq:
        null.add("z_q")
    if not want_loss:
        null |= {"loss", "ws_vq"}
    if hist is None:
        null.add("hist")
    if not decode:
        null |= {"dind", "dmask_c", "dmask_m", "dmask_f", "dz_q", "status", "ws_decompress"}
    if ws_refine is None:
        null.add("ws_refine")
    return null


@pytest.mark.parametrize("decode, x_out, want_zq, want_loss, with_hist, with_refine", list(itertools.product([True, False], repeat=6)))
def test_every_field_points_at_a_buffer_of_its_size_or_is_null(decode, x_out, want_zq, want_loss, with_hist, with_refine):
    made = []

    def alloc(shape, dtype):
        made.append(torch.empty(shape, dtype=dtype))
        return made[-1]

    hist = torch.zeros(1024, dtype=torch.int64) if with_hist else None
    ws_refine = torch.empty(4096, dtype=torch.uint8) if with_refine else None
    t, io = image_io_buffers(SLOT, B, H, W, decode, x_out, want_zq, want_loss, hist, alloc, ws_refine=ws_refine)
    size_at = {m.data_ptr(): m.numel() * m.element_size() for m in made + [m for m in (hist, ws_refine) if m is not None]}
    assert len(size_at) == len(made) + with_hist + with_refine and 0 not in size_at
    want, null = expected_bytes(hist, ws_refine), expected_null(decode, x_out, want_zq, want_loss, hist, ws_refine)
    pointers = [f for f in FIELDS if f not in ("x_is_u8", "slot", "ws_refine_bytes")]
    assert {f for f in pointers if not getattr(io, f)} == null
    spans = []
    for f in pointers:
        if f in null:
            continue
        ptr = getattr(io, f)
        assert size_at.get(ptr) == want[f], f
        spans.append((ptr, ptr + want[f], f))
    spans.sort()
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        assert end <= start, f"{a} and {b} overlap"
    assert io.slot == SLOT and io.x_is_u8 == 0
    assert io.ws_refine_bytes == (4096 if with_refine else 0)
    # every buffer the struct points at is held by the returned dict (or is the caller's own)
    held = {m.data_ptr() for v in t.values() for m in (v if isinstance(v, list) else [v]) if isinstance(m, torch.Tensor)}
    assert {getattr(io, f) for f in pointers if f not in null} <= held
    assert hist is None or io.hist == hist.data_ptr()
    assert ws_refine is None or io.ws_refine == ws_refine.data_ptr()
    # the names the two callers read results by
    assert [tuple(m.shape) for m in t["mask"]] == [(B, 1, h // 4, w // 4), (B, 1, h // 2, w // 2), (B, 1, h, w)]
    assert tuple(t["data"].shape) == (B, 5, SLOT) and tuple(t["nbytes"].shape) == (B, 5) and tuple(t["ind"].shape) == (B * h * w,)
    if decode:
        assert tuple(t["dind"].shape) == (B, h, w) and tuple(t["dz_q"].shape) == (B, 4, h, w) and tuple(t["status"].shape) == (B,)


def test_grain_masks_are_the_routers_three_int32_layouts():
    for m, shape in zip(_lib.grain_masks(3, 16, 24, "cpu"), [(3, 1, 4, 6), (3, 1, 8, 12), (3, 1, 16, 24)]):
        assert tuple(m.shape) == shape and m.dtype == torch.int32 and m.is_contiguous()
    assert cg._lib.grain_masks(1, 4, 4, alloc=lambda s, d: (s, d)) == [((1, 1, 1, 1), torch.int32), ((1, 1, 2, 2), torch.int32),
                                                                       ((1, 1, 4, 4), torch.int32)]
