"""GPU: the merge, the pools and the blends on fp16 / bf16 features (the _h calls of csrc/cgic_merge.hip, ABI 16) against values computed ON THE
CPU: the reference's own expressions on CPU half tensors for the merge and the blends (they promote to fp32, the masks being
.float(); `.to(half)` of that where the half output is asked for), torch's CPU avg_pool2d on the half tensor for the pools.
Everything is compared bit for bit; where the expected value is a NaN, a NaN is expected (payloads are not compared)."""
import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib, merge
from control_gic_amd import model as cgmodel

pytestmark = pytest.mark.gpu
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
HALVES = [pytest.param(f16, id="fp16"), pytest.param(bf16, id="bf16")]


@pytest.fixture(scope="module", autouse=True)
def abi_16():
    """first of all: on an older library every test fails HERE, and no fp32 kernel is ever pointed at a half-sized buffer"""
    assert _lib.lib().cgic_abi_version() >= 16


# ---------------------------------------------------------------------------- the reference (restated from test_training_kernels.py)
def up(t, k):
    return torch.nn.Upsample(scale_factor=k, mode="nearest")(t) if t.numel() else t.repeat_interleave(k, -2).repeat_interleave(k, -1)


# the router's seven modes = the non-empty subsets of {coarse, medium, fine} that a batch is routed to; "overlap": independent
# 0/1 masks (no router makes them; the kernels are products and sums and must follow the expression there too)
MODES = ["cmf", "cm", "cf", "mf", "c", "m", "f", "overlap"]


def make_masks(mode, B, h, w, seed=0):
    """int32 masks [B,1,h/4,w/4], [B,1,h/2,w/2], [B,1,h,w]: exclusive (every fine position routed to exactly one grain), or independent"""
    rng = np.random.default_rng([seed, B, h, w, MODES.index(mode)])
    if mode == "overlap":
        return [torch.from_numpy(rng.integers(0, 2, (B, 1, h // s, w // s)).astype(np.int32)) for s in (4, 2, 1)]
    rep = lambda a, k: a.repeat(k, -2).repeat(k, -1)
    mc = (rng.random((B, 1, h // 4, w // 4)) < 0.4) if "c" in mode and len(mode) > 1 else np.full((B, 1, h // 4, w // 4), mode == "c")
    mm = (rng.random((B, 1, h // 2, w // 2)) < 0.5) if "m" in mode and "f" in mode else np.full((B, 1, h // 2, w // 2), "m" in mode)
    mm &= ~rep(mc, 2)
    mf = ~rep(mc, 4) & ~rep(mm, 2)
    assert (rep(mc, 4).astype(int) + rep(mm, 2) + mf == 1).all()
    return [torch.from_numpy(np.ascontiguousarray(m).astype(np.int32)) for m in (mc, mm, mf)]


def ref_merge(hc, hm, hf, mk):
    return up(hc, 4) * up(mk[0].float(), 4) + up(hm, 2) * up(mk[1].float(), 2) + hf * mk[2]               # vqvae_blocks.py:364-366


def ref_blend_medium(hin, own, mk):
    return hin * up(mk[0].float(), 2) + own * mk[1]                                                     # decoder.py:373-374


def ref_blend_fine(hin, own, mk):
    return hin * up(mk[0].float(), 4) + hin * up(mk[1].float(), 2) + own * mk[2]                          # decoder.py:376-378


def ref_pool(x, k):
    return torch.nn.functional.avg_pool2d(x, k, k, 0) if x.numel() else x.new_empty(*x.shape[:2], x.shape[2] // k, x.shape[3] // k)


def same_bits(got, want):
    """the same type and shape, NaNs in the same places, the same bit patterns everywhere else"""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (got.dtype, want.dtype, got.shape, want.shape)
    as_int = torch.int32 if want.dtype == f32 else torch.int16
    g, w = got.cpu().contiguous(), want.contiguous()
    gn, wn = torch.isnan(g), torch.isnan(w)
    assert torch.equal(gn, wn), f"{int((gn != wn).sum())} NaN positions differ"
    diff = (g.view(as_int) != w.view(as_int)) & ~wn
    assert not bool(diff.any()), f"{int(diff.sum())} of {diff.numel()} bit patterns differ, first at {diff.nonzero()[0].tolist()}"


def cuda(ts):
    return [t.cuda() for t in ts]


def randn(gen, dtype, *shape):
    return torch.randn(*shape, generator=gen).to(dtype)


def expect(ref32, dtype, to_half):
    """the reference's fp32 tensor, or what `.to(half)` makes of it"""
    assert ref32.dtype == f32
    return ref32.to(dtype) if to_half else ref32


def check_streams(B, C, h, w, mode, dtype, seed=0, plant=None):
    """grain merge + fine blend on the fine grid [B,C,h,w], medium blend on [B,C,h/2,w/2], both pools, both output types, in place
    and into a given fp32 tensor"""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * B + C + h + w)
    mk = make_masks(mode, B, h, w, seed)
    hc, hm, hf, own = (randn(gen, dtype, B, C, h // 4, w // 4), randn(gen, dtype, B, C, h // 2, w // 2), randn(gen, dtype, B, C, h, w),
                       randn(gen, dtype, B, C, h, w))
    own_m = randn(gen, dtype, B, C, h // 2, w // 2)
    if plant is not None:
        plant(mk, hc, hm, hf, own, own_m)
    dmk = cuda(mk)
    want_merge, want_fine, want_medium = ref_merge(hc, hm, hf, mk), ref_blend_fine(hf, own, mk), ref_blend_medium(hm, own_m, mk[:2])
    for to_half in (False, True):
        kw = {"out_dtype": dtype} if to_half else {}
        same_bits(cg.grain_merge(*cuda((hc, hm, hf)), dmk, **kw), expect(want_merge, dtype, to_half))
        same_bits(merge.decoder_blend_fine(*cuda((hf, own)), *dmk, **kw), expect(want_fine, dtype, to_half))
        same_bits(cg.decoder_blend_medium(*cuda((hm, own_m)), dmk[:2], **kw), expect(want_medium, dtype, to_half))
    buf = hf.cuda()
    assert cg.decoder_blend_fine(buf, own.cuda(), dmk, out=buf) is buf                                   # in place: half in, half out
    same_bits(buf, want_fine.to(dtype))
    buf = hm.cuda()
    assert cg.decoder_blend_medium(buf, own_m.cuda(), dmk[:2], out=buf) is buf
    same_bits(buf, want_medium.to(dtype))
    out = torch.full((B, C, h, w), 7.0, device="cuda")                                                  # into a given fp32 tensor
    assert cg.decoder_blend_fine(hf.cuda(), own.cuda(), dmk, out=out) is out
    same_bits(out, want_fine)
    out = torch.full((B, C, h // 2, w // 2), 7.0, device="cuda")
    assert cg.decoder_blend_medium(hm.cuda(), own_m.cuda(), dmk[:2], out=out) is out
    same_bits(out, want_medium)
    for k in (2, 4):
        same_bits(merge.avg_pool(hf.cuda(), k, out_dtype=dtype), ref_pool(hf, k))                        # AvgPool2d keeps the type
        same_bits(merge.avg_pool(hf.cuda(), k), ref_pool(hf.float(), k))                                 # fp32 out: the fp32 kernel on the upcast
    return mk, hc, hm, hf, own, own_m


# fine widths 4, 8, 4, 20, 16, 24: the 4- and the 8-element unit with one to five threads per row; medium grids 2, 4, 2, 10, 8, 12 wide:
# the 2-, 4- and 8-element unit; pools of 2 x 2 and 4 x 4 windows with 1, 2 and 4 outputs per thread; an empty batch
SHAPES = [(1, 1, 4, 4), (2, 3, 4, 8), (1, 2, 8, 4), (2, 1, 12, 20), (1, 2, 8, 16), (2, 3, 8, 24), (0, 3, 8, 8)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,h,w", SHAPES)
@pytest.mark.parametrize("dtype", HALVES)
def test_streams_small_shapes_in_every_mode(dtype, B, C, h, w, mode):
    check_streams(B, C, h, w, mode, dtype)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,hh,ww", [(2, 2, 4, 2), (1, 3, 6, 6), (2, 1, 2, 6)])
@pytest.mark.parametrize("dtype", HALVES)
def test_medium_blend_on_grids_2_and_6_wide(dtype, B, C, hh, ww, mode):
    """the 2-element unit with one and three threads per row"""
    gen = torch.Generator().manual_seed(hh * ww)
    mk = make_masks(mode, B, 2 * hh, 2 * ww)[:2]
    hin, own = randn(gen, dtype, B, C, hh, ww), randn(gen, dtype, B, C, hh, ww)
    want = ref_blend_medium(hin, own, mk)
    same_bits(cg.decoder_blend_medium(hin.cuda(), own.cuda(), cuda(mk), out_dtype=f32), want)
    same_bits(cg.decoder_blend_medium(hin.cuda(), own.cuda(), cuda(mk), out_dtype=dtype), want.to(dtype))


# ---------------------------------------------------------------------------- pointers that allow only a narrower unit
def offset_view(t, elements):
    """t's values in a device tensor whose storage begins `elements` elements before it: a contiguous view at that storage offset"""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device="cuda")
    v = buf[elements:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == elements and v.data_ptr() % 16 == (2 * elements) % 16
    return v


@pytest.mark.parametrize("elements", [4, 2, 1])
@pytest.mark.parametrize("dtype", HALVES)
def test_a_feature_tensor_at_a_storage_offset_takes_the_narrower_unit(dtype, elements):
    """widths that allow 8 elements per thread, a pointer that is aligned to 8, 4 or 2 bytes only: the 4-, 2- or 1-element unit (the
    plan: tests/test_merge_plan_host.py) -- for each feature in turn, and for `out`"""
    B, C, h, w = 2, 3, 8, 16
    gen = torch.Generator().manual_seed(elements)
    mk = make_masks("cmf", B, h, w)
    hc, hm, hf, own = (randn(gen, dtype, B, C, h // 4, w // 4), randn(gen, dtype, B, C, h // 2, w // 2), randn(gen, dtype, B, C, h, w),
                       randn(gen, dtype, B, C, h, w))
    dmk = cuda(mk)
    want_merge, want_fine = ref_merge(hc, hm, hf, mk), ref_blend_fine(hf, own, mk)
    for which in range(3):
        feats = [offset_view(t, elements) if i == which else t.cuda() for i, t in enumerate((hc, hm, hf))]
        same_bits(cg.grain_merge(*feats, dmk), want_merge)
    same_bits(cg.decoder_blend_fine(offset_view(hf, elements), own.cuda(), dmk, out_dtype=dtype), want_fine.to(dtype))
    same_bits(cg.decoder_blend_fine(hf.cuda(), offset_view(own, elements), dmk, out_dtype=f32), want_fine)
    out = offset_view(torch.zeros(B, C, h, w, dtype=dtype), elements)
    assert cg.decoder_blend_fine(hf.cuda(), own.cuda(), dmk, out=out) is out
    same_bits(out, want_fine.to(dtype))
    buf = offset_view(hf, elements)                                                                       # in place at the offset
    cg.decoder_blend_fine(buf, own.cuda(), dmk, out=buf)
    same_bits(buf, want_fine.to(dtype))
    hm_own = randn(gen, dtype, B, C, h // 2, w // 2)
    same_bits(cg.decoder_blend_medium(offset_view(hm, elements), hm_own.cuda(), dmk[:2], out_dtype=dtype),
              ref_blend_medium(hm, hm_own, mk[:2]).to(dtype))
    for k in (2, 4):
        same_bits(merge.avg_pool(offset_view(hf, elements), k, out_dtype=dtype), ref_pool(hf, k))


# ---------------------------------------------------------------------------- past the grid caps
# 8 elements per thread, 256 threads, 8192 workgroups for the merge and 16384 for the others; 33 (65 for the pool) threads per row,
# so that the grid stride wraps in the middle of a row
def test_grain_merge_beyond_its_grid_cap():
    B, C, h, w = 1, 129, 512, 264
    assert B * C * h * w > 8192 * 256 * 8 and (w // 8) % 2 == 1
    gen = torch.Generator().manual_seed(1)
    mk = make_masks("cmf", B, h, w)
    hc, hm, hf = randn(gen, bf16, B, C, h // 4, w // 4), randn(gen, bf16, B, C, h // 2, w // 2), randn(gen, bf16, B, C, h, w)
    same_bits(cg.grain_merge(*cuda((hc, hm, hf)), cuda(mk)), ref_merge(hc, hm, hf, mk))


@pytest.mark.parametrize("which,dtype", [("fine", f16), ("medium", bf16)])
def test_blends_beyond_the_grid_cap(which, dtype):
    B, C, h, w = 2, 130, 512, 264
    assert B * C * h * w > 16384 * 256 * 8 and (w // 8) % 2 == 1
    gen = torch.Generator().manual_seed(w)
    hin, own = randn(gen, dtype, B, C, h, w), randn(gen, dtype, B, C, h, w)
    if which == "fine":
        mk = make_masks("cmf", B, h, w)
        same_bits(cg.decoder_blend_fine(hin.cuda(), own.cuda(), cuda(mk), out_dtype=dtype), ref_blend_fine(hin, own, mk).to(dtype))
    else:
        mk = make_masks("cmf", B, 2 * h, 2 * w)[:2]
        same_bits(cg.decoder_blend_medium(hin.cuda(), own.cuda(), cuda(mk), out_dtype=f32), ref_blend_medium(hin, own, mk))


def test_avg_pool_beyond_the_grid_cap():
    C, H, W, k = 253, 512, 520, 2
    assert C * (H // k) * (W // 8) > 16384 * 256 and (W // 8) % 2 == 1                                    # four outputs per thread
    x = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(k)).to(f16)
    same_bits(merge.avg_pool(x.cuda(), k, out_dtype=f16), ref_pool(x, k))


# ---------------------------------------------------------------------------- special values
def specials(dtype):
    fi = torch.finfo(dtype)
    sub = [2.0 ** -24, 1.0e-6] if dtype == f16 else [2.0 ** -133, 1.0e-39]                               # subnormals of the type
    return [np.inf, -np.inf, np.nan, -0.0, fi.max, -fi.max] + sub + [-sub[0]]


def _plant(t, selected, values):
    """every special value once where `selected` (broadcast to t) is set and once where it is not"""
    sel = selected.expand_as(t).reshape(-1)
    on, off = torch.nonzero(sel).reshape(-1), torch.nonzero(~sel).reshape(-1)
    assert len(on) >= len(values) and len(off) >= len(values)
    step_on, step_off = len(on) // len(values), len(off) // len(values)
    for i, v in enumerate(values):
        t.view(-1)[on[i * step_on]] = v
        t.view(-1)[off[i * step_off]] = v


@pytest.mark.parametrize("mode", ["cmf", "overlap"])
@pytest.mark.parametrize("dtype", HALVES)
def test_streams_special_values_in_selected_and_masked_out_positions(dtype, mode):
    """products and sums, not selects: an Inf or NaN that the mask zeroes is a NaN in the output like in the reference; -0.0, the
    largest finite values and subnormals come through with their bits (fp16 subnormals are not flushed by the upcast)"""
    vals = specials(dtype)
    sub = torch.tensor(vals[6:8], dtype=dtype)
    assert bool((sub != 0).all()) and bool((sub.float().abs() < torch.finfo(dtype).tiny).all())          # subnormal in the type, kept by this host

    def plant(mk, hc, hm, hf, own, own_m):
        b = [m.bool() for m in mk]
        _plant(hc, b[0], vals)
        _plant(hm, b[1], vals)
        _plant(hf, b[2], vals)
        _plant(own, b[2], vals)
        _plant(own_m, b[1], vals)

    mk, hc, hm, hf, own, own_m = check_streams(2, 3, 16, 24, mode, dtype, seed=3, plant=plant)
    ref = ref_merge(hc, hm, hf, mk)
    if mode == "cmf":
        assert bool(torch.isnan(ref).any()) and bool((ref.abs() == float(sub[0])).any()) and bool(torch.isinf(ref).any())
    zeroed_inf = torch.isinf(hf) & (mk[2] == 0)
    assert bool(zeroed_inf.any()) and bool(torch.isnan(ref[zeroed_inf]).all())                          # x * 0 with x = Inf


def test_overlapping_masks_whose_fp16_sum_overflows():
    """independent masks: h * 1 + h * 1 + own * 1 of values near 60000 is finite in fp32 and +-Inf once rounded to fp16, as
    `.to(torch.float16)` makes it"""
    B, C, h, w = 2, 2, 8, 16
    gen = torch.Generator().manual_seed(5)
    mk = make_masks("overlap", B, h, w, seed=1)
    big = lambda *s: (torch.randint(0, 2, s, generator=gen).float() * 2 - 1) * (60000.0 - 32.0 * torch.randint(0, 8, s, generator=gen).float())
    hc, hm, hf, own = big(B, C, h // 4, w // 4).to(f16), big(B, C, h // 2, w // 2).to(f16), big(B, C, h, w).to(f16), big(B, C, h, w).to(f16)
    dmk = cuda(mk)
    for want, got32, got16 in (
            (ref_merge(hc, hm, hf, mk), cg.grain_merge(*cuda((hc, hm, hf)), dmk), cg.grain_merge(*cuda((hc, hm, hf)), dmk, out_dtype=f16)),
            (ref_blend_fine(hf, own, mk), cg.decoder_blend_fine(hf.cuda(), own.cuda(), dmk, out_dtype=f32),
             cg.decoder_blend_fine(hf.cuda(), own.cuda(), dmk, out_dtype=f16))):
        assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 100000.0
        assert bool(torch.isinf(want.to(f16)).any()) and bool((want.to(f16) == np.inf).any()) and bool((want.to(f16) == -np.inf).any())
        same_bits(got32, want)
        same_bits(got16, want.to(f16))


@pytest.mark.parametrize("dtype", HALVES)
def test_avg_pool_accumulates_in_fp32_and_rounds_once(dtype):
    """the window's fp32 row-major running sum: two fp16 values of 60000 average to 30000 (k = 2); four of the largest bf16 values
    overflow the fp32 sum; windows of subnormals average to subnormals; a negative average that underflows is +0 like ATen's"""
    fi = torch.finfo(dtype)
    big = 60000.0 if dtype == f16 else 3.0e38
    tiny = 2.0 ** -24 if dtype == f16 else 2.0 ** -133
    for k in (2, 4):
        x = randn(torch.Generator().manual_seed(k), dtype, 2, 3, 4 * k, 8 * k)
        win = lambda i, j: x[0, 0, i * k:(i + 1) * k, j * k:(j + 1) * k]
        win(0, 0)[:] = 0.0; win(0, 0)[0, 0] = big; win(0, 0)[0, 1] = big
        win(0, 1)[:] = big
        win(0, 2)[:] = fi.max
        win(0, 3)[:] = -fi.max
        win(0, 4)[:] = 0.0; win(0, 4)[0, 0] = fi.max; win(0, 4)[0, 1] = fi.max; win(0, 4)[1, 0] = -fi.max; win(0, 4)[1, 1] = -fi.max
        win(0, 5)[:] = 0.0; win(0, 5)[0, 0] = fi.max; win(0, 5)[1, 0] = fi.max; win(0, 5)[0, 1] = -fi.max; win(0, 5)[1, 1] = -fi.max
        win(1, 0)[:] = tiny
        win(1, 1)[:] = 3 * tiny
        win(1, 2)[:] = 0.0; win(1, 2)[0, 0] = tiny                                                       # underflows to +0
        win(1, 3)[:] = 0.0; win(1, 3)[0, 0] = -tiny                                                      # a negative average that underflows
        win(1, 4)[:] = -0.0
        win(1, 5)[:] = -tiny; win(1, 5)[0, 0] = -0.0
        win(2, 0)[0, 0] = np.inf; win(2, 0)[-1, -1] = -np.inf
        win(2, 1)[-1, -1] = np.nan
        win(2, 2)[0, 1] = np.inf
        win(2, 3)[:] = fi.tiny
        x[1, 2] = (torch.randn(4 * k, 8 * k, generator=torch.Generator().manual_seed(9)) * 4 * tiny).to(dtype)
        ref = ref_pool(x, k)
        if dtype == f16:
            assert float(ref[0, 0, 0, 0]) == 120000.0 / (k * k) and float(ref[0, 0, 0, 1]) == 60000.0 and float(ref[0, 0, 0, 2]) == 65504.0
        else:
            assert float(ref[0, 0, 0, 2]) == np.inf and float(ref[0, 0, 0, 3]) == -np.inf
        assert float(ref[0, 0, 1, 0]) == tiny and float(ref[0, 0, 1, 1]) == 3 * tiny
        assert ref[0, 0, 1, 3].view(torch.int16).item() == 0 and torch.isnan(ref[0, 0, 2, 0]) and torch.isnan(ref[0, 0, 2, 1])
        same_bits(merge.avg_pool(x.cuda(), k, out_dtype=dtype), ref)
        same_bits(cgmodel.AvgPool(k)(x.cuda()), ref)
        same_bits(merge.avg_pool(x.cuda(), k), ref_pool(x.float(), k))


# ---------------------------------------------------------------------------- the module, the ops and their gradients
@pytest.mark.parametrize("dtype", HALVES)
def test_avgpool_module_keeps_the_type_of_a_half_input(dtype):
    x = randn(torch.Generator().manual_seed(3), dtype, 2, 5, 16, 24)
    for k in (2, 4):
        pool = cgmodel.AvgPool(k)
        y = pool(x.cuda())
        assert y.dtype == dtype and tuple(y.shape) == (2, 5, 16 // k, 24 // k)
        same_bits(y, ref_pool(x, k))
        with torch.no_grad():
            same_bits(pool(x.cuda().requires_grad_()), ref_pool(x, k))
        xg = x.cuda().requires_grad_()                                                                    # autograd needed: torch's own pool
        yg = pool(xg)
        assert yg.dtype == dtype and yg.requires_grad
        yg.float().sum().backward()
        assert xg.grad is not None and xg.grad.dtype == dtype
        with torch.autocast("cuda", dtype=dtype):
            same_bits(pool(x.cuda()), ref_pool(x, k))


def _unit_roundoff(dtype):
    return 2.0 ** -11 if dtype == f16 else 2.0 ** -8


@pytest.mark.parametrize("dtype", HALVES)
def test_the_ops_on_half_inputs_return_fp32_and_carry_gradients(dtype):
    """torch.ops.cgic.* keep their schemas: fp32 out with the reference's bits, through the half kernels.  Gradients against fp64
    autograd of the expression on the same (exactly upcast) inputs: the incoming gradient is fp32, the formulas are g x mask
    (exact) and window sums of g (each fp32 window sum within (k^2 - 1) 2^-24 sum |g|, the bound of the fp32 gradient tests); the
    result is then rounded once to the leaf's half type: u |value| more, u = 2^-11 (fp16) or 2^-8 (bf16)."""
    B = C = 3
    h, w = 8, 16
    gen = torch.Generator().manual_seed(41)
    mk = make_masks("cmf", B, h, w, seed=2)
    dmk = cuda(mk)
    ts = [randn(gen, dtype, B, C, h // 4, w // 4), randn(gen, dtype, B, C, h // 2, w // 2), randn(gen, dtype, B, C, h, w)]
    wgt = torch.randn(B, C, h, w, generator=gen)
    u = _unit_roundoff(dtype)

    def close(got, want64, window_tol=0.0):
        assert got.dtype == dtype
        err = (got.cpu().double() - want64).abs()
        bound = (want64.abs() + window_tol) * u + window_tol
        assert bool((err <= bound).all()), float((err - bound).max())

    def window_tol(k):
        return (k * k - 1) * 2.0 ** -24 * torch.nn.functional.avg_pool2d(wgt.double().abs(), k, k, 0) * (k * k)

    a, b = [t.cuda().requires_grad_() for t in ts], [t.double().requires_grad_() for t in ts]
    out = torch.ops.cgic.grain_merge(a[0], a[1], a[2], *dmk)
    same_bits(out.detach(), ref_merge(*ts, mk))
    (out * wgt.cuda()).sum().backward()
    (ref_merge(b[0], b[1], b[2], [m.double() for m in mk]) * wgt.double()).sum().backward()
    close(a[2].grad, b[2].grad)
    close(a[1].grad, b[1].grad, window_tol(2) * mk[1].double())
    close(a[0].grad, b[0].grad, window_tol(4) * mk[0].double())
    assert bool((a[0].grad.cpu()[(mk[0] == 0).expand_as(ts[0])] == 0).all())

    hin, own = ts[2], randn(gen, dtype, B, C, h, w)
    a, b = [t.cuda().requires_grad_() for t in (hin, own)], [t.double().requires_grad_() for t in (hin, own)]
    out = torch.ops.cgic.decoder_blend_fine(a[0], a[1], *dmk)
    same_bits(out.detach(), ref_blend_fine(hin, own, mk))
    (out * wgt.cuda()).sum().backward()
    (ref_blend_fine(b[0], b[1], [m.double() for m in mk]) * wgt.double()).sum().backward()
    close(a[0].grad, b[0].grad)
    close(a[1].grad, b[1].grad)

    mk2 = make_masks("overlap", B, 2 * h, 2 * w, seed=4)[:2]
    a, b = [t.cuda().requires_grad_() for t in (hin, own)], [t.double().requires_grad_() for t in (hin, own)]
    out = torch.ops.cgic.decoder_blend_medium(a[0], a[1], *cuda(mk2))
    same_bits(out.detach(), ref_blend_medium(hin, own, mk2))
    (out * wgt.cuda()).sum().backward()
    (ref_blend_medium(b[0], b[1], [m.double() for m in mk2]) * wgt.double()).sum().backward()
    close(a[0].grad, b[0].grad)
    close(a[1].grad, b[1].grad)

    for k in (2, 4):
        a, b = hin.cuda().requires_grad_(), hin.double().requires_grad_()
        out = torch.ops.cgic.avg_pool(a, k)
        same_bits(out.detach(), ref_pool(hin.float(), k))
        wk = torch.randn(B, C, h // k, w // k, generator=gen)
        (out * wk.cuda()).sum().backward()
        (torch.nn.functional.avg_pool2d(b, k, k, 0) * wk.double()).sum().backward()
        close(a.grad, b.grad)


@pytest.mark.parametrize("dtype", HALVES)
def test_a_blend_with_out_given_allocates_nothing(dtype):
    """no cast temporary: the caching allocator's allocation count does not move across the call"""
    B, C, h, w = 2, 4, 16, 32
    gen = torch.Generator().manual_seed(2)
    dmk = cuda(make_masks("cmf", B, h, w))
    hf, own, out32 = randn(gen, dtype, B, C, h, w).cuda(), randn(gen, dtype, B, C, h, w).cuda(), torch.empty(B, C, h, w, device="cuda")
    hm, own_m = randn(gen, dtype, B, C, h // 2, w // 2).cuda(), randn(gen, dtype, B, C, h // 2, w // 2).cuda()
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    for call in (lambda: cg.decoder_blend_fine(hf, own, dmk, out=out32), lambda: cg.decoder_blend_fine(hf, own, dmk, out=hf),
                 lambda: cg.decoder_blend_medium(hm, own_m, dmk[:2], out=hm)):
        torch.cuda.synchronize()
        before = count()
        call()
        assert count() == before


def test_fp32_inputs_take_the_fp32_path_as_before():
    """(a guard: fp32 in, fp32 out, the reference's bits -- also with out_dtype named)"""
    B, C, h, w = 2, 3, 8, 16
    gen = torch.Generator().manual_seed(8)
    mk = make_masks("cmf", B, h, w)
    dmk = cuda(mk)
    hc, hm, hf, own = (randn(gen, f32, B, C, h // 4, w // 4), randn(gen, f32, B, C, h // 2, w // 2), randn(gen, f32, B, C, h, w),
                       randn(gen, f32, B, C, h, w))
    same_bits(cg.grain_merge(*cuda((hc, hm, hf)), dmk), ref_merge(hc, hm, hf, mk))
    same_bits(merge.grain_merge(*cuda((hc, hm, hf)), *dmk, out_dtype=f32), ref_merge(hc, hm, hf, mk))
    same_bits(cg.decoder_blend_fine(hf.cuda(), own.cuda(), dmk), ref_blend_fine(hf, own, mk))
    same_bits(cg.decoder_blend_medium(hm.cuda(), hm.cuda(), dmk[:2]), ref_blend_medium(hm, hm, mk[:2]))
    for k in (2, 4):
        same_bits(cg.avg_pool(hf.cuda(), k), ref_pool(hf, k))
    mixed = cg.decoder_blend_fine(hf.cuda().to(bf16), own.cuda(), dmk)                                    # a mixture: cast to fp32, as before
    same_bits(mixed, ref_blend_fine(hf.to(bf16).float(), own, mk))
