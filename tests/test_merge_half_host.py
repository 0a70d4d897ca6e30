"""CPU: the half-precision merge / pool / blend path (ABI 16) as far as it goes without a device.

  - the shape of the ABI: the four _h entry points in the header, the library and the ctypes table;
  - what merge.py and model.py refuse, with the full message, under FakeTensorMode on fake "cuda" tensors (every check sits in front of
    the first data_ptr(), as in test_python_refusals_host.py);
  - which entry point a call reaches: fp32 features the _f32 one, features all of one half type the _h one with no cast, any
    mixture the _f32 one through casts (the library call itself is replaced by a recorder);
  - the CPU statement that DEFINES the half pool's value: torch's CPU avg_pool2d on fp16 / bf16 is the fp32 row-major running sum of
    the window, divided by k^2 in fp32, rounded once to nearest-even -- with one addition found while writing it down: a result
    of -0 (a negative average that underflows the half type) comes out as +0."""
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib, merge, model as cgmodel

f32, f16, bf16, f64, i32 = torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLEND_M = "decoder_blend_medium: h, h_medium on the medium grid; mask_c at half of it, mask_m on it"
B, C, H, W = 2, 8, 16, 24
NEW = {"cgic_grain_merge_h": 14, "cgic_avgpool_h": 9, "cgic_decoder_blend_medium_h": 12, "cgic_decoder_blend_fine_h": 13}


# ---------------------------------------------------------------------------- the ABI
def test_abi_16_declares_exports_and_binds_the_four_half_entry_points():
    assert _lib.lib().cgic_abi_version() >= 16
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgic_hip.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr).group(1)
        assert len(args.split(",")) == nargs, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert [int(re.search(r"#define\s+CGIC_DT_" + n + r"\s+(\d+)", hdr).group(1)) for n in ("F32", "F16", "BF16")] == [0, 1, 2]
    assert merge._DT == {f32: 0, f16: 1, bf16: 2}


def test_the_library_refuses_before_it_launches():
    """the entry points check, then plan, then launch: a refused call enqueues nothing, so it can be made without a device and with
    made-up addresses (never dereferenced).  The plan's full table: tests/test_merge_plan_host.py"""
    A, Bm, Cm, M0, M1, M2, OUT = (0x10000000 + i * 0x1000000 for i in range(7))

    def refused(code, text, name, *args):
        with pytest.raises(cg.CgicError) as got:
            _lib.call(name, *args)
        assert got.value.code == code and text in str(got.value), str(got.value)

    refused(_lib.ERR_UNSUPPORTED, "grain_merge: fp32 features are cgic_grain_merge_f32's", "cgic_grain_merge_h", A, Bm, Cm, 0, M0, M1, M2, 1, 3, 8, 8, OUT, 0, None)
    refused(_lib.ERR_UNSUPPORTED, "avgpool: fp32 features are cgic_avgpool_f32's", "cgic_avgpool_h", A, 0, 3, 8, 8, 2, OUT, 0, None)
    refused(_lib.ERR_UNSUPPORTED, "decoder_blend_medium: fp32 features are cgic_decoder_blend_medium_f32's", "cgic_decoder_blend_medium_h",
            A, Bm, 0, M0, M1, 1, 3, 8, 8, OUT, 0, None)
    refused(_lib.ERR_UNSUPPORTED, "decoder_blend_fine: fp32 features are cgic_decoder_blend_fine_f32's", "cgic_decoder_blend_fine_h",
            A, Bm, 0, M0, M1, M2, 1, 3, 8, 8, OUT, 0, None)
    refused(_lib.ERR_UNSUPPORTED, "out_dtype 2 with in_dtype 1", "cgic_avgpool_h", A, 1, 3, 8, 8, 2, OUT, 2, None)
    refused(_lib.ERR_UNSUPPORTED, "avgpool: window 3", "cgic_avgpool_h", A, 1, 3, 9, 9, 3, OUT, 1, None)
    refused(_lib.ERR_INVALID, "avgpool: 8x7 is not a multiple of the window", "cgic_avgpool_h", A, 2, 3, 8, 7, 2, OUT, 2, None)
    refused(_lib.ERR_INVALID, "grain_merge: fine grid 6x8 must be positive multiples of 4", "cgic_grain_merge_h", A, Bm, Cm, 1, M0, M1, M2, 1, 3,
            6, 8, OUT, 0, None)
    refused(_lib.ERR_INVALID, "decoder_blend_medium: medium grid 3x4 (need even height and width)", "cgic_decoder_blend_medium_h", A, Bm, 2, M0,
            M1, 1, 3, 3, 4, OUT, 2, None)
    refused(_lib.ERR_INVALID, "decoder_blend_fine: NULL tensor", "cgic_decoder_blend_fine_h", A, Bm, 1, M0, M1, None, 1, 3, 8, 8, OUT, 0, None)
    refused(_lib.ERR_INVALID, "a pointer is not aligned to its 2-byte element", "cgic_decoder_blend_fine_h", A + 1, Bm, 1, M0, M1, M2, 1, 3, 8, 8,
            OUT, 0, None)
    refused(_lib.ERR_INVALID, "decoder_blend_fine: out overlaps an input", "cgic_decoder_blend_fine_h", A, Bm, 1, M0, M1, M2, 1, 3, 8, 8, A, 0, None)
    refused(_lib.ERR_INVALID, "decoder_blend_fine: out overlaps an input", "cgic_decoder_blend_fine_h", A, Bm, 1, M0, M1, M2, 1, 3, 8, 8, Bm, 1, None)
    refused(_lib.ERR_INVALID, "grain_merge: out overlaps an input", "cgic_grain_merge_h", A, Bm, Cm, 2, M0, M1, M2, 1, 3, 8, 8, Cm, 2, None)
    # the _f32 calls go through the same plan: the texts they have always had ...
    refused(_lib.ERR_UNSUPPORTED, "avgpool: window 3; the decoder uses 4 and 2 (decoder.py:304-305)", "cgic_avgpool_f32", A, 3, 9, 9, 3, OUT, None)
    refused(_lib.ERR_INVALID, "avgpool: 8x7 is not a multiple of the window", "cgic_avgpool_f32", A, 3, 8, 7, 2, OUT, None)
    refused(_lib.ERR_INVALID, "grain_merge: fine grid 6x8 must be positive multiples of 4", "cgic_grain_merge_f32", A, Bm, Cm, M0, M1, M2, 1, 3, 6, 8,
            OUT, None)
    refused(_lib.ERR_INVALID, "decoder_blend_medium: medium grid 3x4 (need even height and width)", "cgic_decoder_blend_medium_f32", A, Bm, M0, M1,
            1, 3, 3, 4, OUT, None)
    refused(_lib.ERR_INVALID, "decoder_blend_fine: fine grid 8x10 must be positive multiples of 4", "cgic_decoder_blend_fine_f32", A, Bm, M0, M1, M2,
            1, 3, 8, 10, OUT, None)
    refused(_lib.ERR_INVALID, "decoder_blend_fine: NULL tensor", "cgic_decoder_blend_fine_f32", A, Bm, M0, M1, None, 1, 3, 8, 8, OUT, None)
    refused(_lib.ERR_INVALID, "grain_merge: NULL tensor", "cgic_grain_merge_f32", A, None, Cm, M0, M1, M2, 1, 3, 8, 8, OUT, None)
    refused(_lib.ERR_INVALID, "avgpool: NULL tensor", "cgic_avgpool_f32", A, 3, 8, 8, 2, None, None)
    # ... and the two that the plan added to them: the pointers' alignment and the half calls' aliasing rule
    refused(_lib.ERR_INVALID, "decoder_blend_fine: a pointer is not aligned to its 4-byte element", "cgic_decoder_blend_fine_f32", A + 2, Bm, M0, M1,
            M2, 1, 3, 8, 8, OUT, None)
    refused(_lib.ERR_INVALID, "decoder_blend_medium: out overlaps an input", "cgic_decoder_blend_medium_f32", A, Bm, M0, M1, 1, 3, 8, 8, Bm, None)
    refused(_lib.ERR_INVALID, "grain_merge: out overlaps an input", "cgic_grain_merge_f32", A, Bm, Cm, M0, M1, M2, 1, 3, 8, 8, Cm, None)
    # an empty batch asks for nothing: CGIC_OK with NULL tensors, nothing launched
    assert _lib.call("cgic_grain_merge_h", None, None, None, 1, None, None, None, 0, 3, 8, 8, None, 0, None) == _lib.OK
    assert _lib.call("cgic_avgpool_h", None, 2, 0, 8, 8, 4, None, 2, None) == _lib.OK
    assert _lib.call("cgic_grain_merge_f32", None, None, None, None, None, None, 0, 3, 8, 8, None, None) == _lib.OK
    assert _lib.call("cgic_avgpool_f32", None, 0, 8, 8, 4, None, None) == _lib.OK


# ---------------------------------------------------------------------------- refusals (FakeTensorMode)
def T(*shape, dtype=f32, device="cuda"):
    return torch.empty(shape, dtype=dtype, device=device)


def feat(dtype=f32, h=H, w=W, device="cuda"):
    return T(B, C, h, w, dtype=dtype, device=device)


def masks(h=H, w=W):
    return [T(B, 1, h // 4, w // 4, dtype=i32), T(B, 1, h // 2, w // 2, dtype=i32), T(B, 1, h, w, dtype=i32)]


def _blends(dt_h, dt_own=None):
    """(name, call(out=..., out_dtype=...)) for the four ways into a blend with `out=`: merge.* and model.*, medium and fine"""
    dt_own = dt_h if dt_own is None else dt_own
    return [
        ("decoder_blend_fine", lambda **kw: merge.decoder_blend_fine(feat(dt_h), feat(dt_own), *masks(), **kw)),
        ("decoder_blend_fine", lambda **kw: cgmodel.decoder_blend_fine(feat(dt_h), feat(dt_own), masks(), **kw)),
        ("decoder_blend_medium", lambda **kw: merge.decoder_blend_medium(feat(dt_h), feat(dt_own), *masks(2 * H, 2 * W)[:2], BLEND_M, **kw)),
        ("decoder_blend_medium", lambda **kw: cgmodel.decoder_blend_medium(feat(dt_h), feat(dt_own), masks(2 * H, 2 * W)[:2], **kw)),
    ]


def _rows():
    rows = []
    f32_only = "the result of these features is torch.float32"
    for name, call in _blends(f32):
        rows += [
            (f"{name}: fp32 features, fp16 out", lambda call=call: call(out=feat(f16)), TypeError, f"{name}: out is torch.float16; {f32_only}"),
            (f"{name}: fp32 features, bf16 out", lambda call=call: call(out=feat(bf16)), TypeError, f"{name}: out is torch.bfloat16; {f32_only}"),
            (f"{name}: fp32 features, fp64 out", lambda call=call: call(out=feat(f64)), TypeError, f"{name}: out is torch.float64; {f32_only}"),
            (f"{name}: out of another shape", lambda call=call: call(out=feat(w=W - 4)), ValueError,
             f"{name}: out {(B, C, H, W - 4)} must have h's shape {(B, C, H, W)}"),
            (f"{name}: out with a batch more", lambda call=call: call(out=T(B + 1, C, H, W)), ValueError,
             f"{name}: out {(B + 1, C, H, W)} must have h's shape {(B, C, H, W)}"),
            (f"{name}: strided out", lambda call=call: call(out=T(B, C, H, 2 * W)[..., ::2]), ValueError, f"{name}: out must be contiguous"),
            (f"{name}: permuted out", lambda call=call: call(out=T(B, C, W, H).permute(0, 1, 3, 2)), ValueError, f"{name}: out must be contiguous"),
            (f"{name}: CPU out", lambda call=call: call(out=feat(device="cpu")), ValueError, f"{name}: out is on cpu, h on cuda:0"),
            (f"{name}: fp32 features, out_dtype fp16", lambda call=call: call(out_dtype=f16), TypeError,
             f"{name}: out_dtype torch.float16; expected torch.float32 (the features are not all of one half type)"),
            (f"{name}: out_dtype against out", lambda call=call: call(out=feat(), out_dtype=bf16), TypeError,
             f"{name}: out_dtype torch.bfloat16, but out is torch.float32"),
        ]
    for name, call in _blends(bf16):
        half = "expected torch.float32 or the features' torch.bfloat16"
        rows += [
            (f"{name}: bf16 features, fp16 out", lambda call=call: call(out=feat(f16)), TypeError, f"{name}: out is torch.float16; {half}"),
            (f"{name}: bf16 features, int32 out", lambda call=call: call(out=feat(i32)), TypeError, f"{name}: out is torch.int32; {half}"),
            (f"{name}: bf16 features, out_dtype fp16", lambda call=call: call(out_dtype=f16), TypeError, f"{name}: out_dtype torch.float16; {half}"),
            (f"{name}: bf16 features, out_dtype fp64", lambda call=call: call(out_dtype=f64), TypeError, f"{name}: out_dtype torch.float64; {half}"),
            (f"{name}: bf16 features, bf16 out of another shape", lambda call=call: call(out=feat(bf16, h=H + 4)), ValueError,
             f"{name}: out {(B, C, H + 4, W)} must have h's shape {(B, C, H, W)}"),
            (f"{name}: bf16 features, strided bf16 out", lambda call=call: call(out=T(B, C, H, 2 * W, dtype=bf16)[..., ::2]), ValueError,
             f"{name}: out must be contiguous"),
            (f"{name}: bf16 features, out_dtype fp32 against a bf16 out", lambda call=call: call(out=feat(bf16), out_dtype=f32), TypeError,
             f"{name}: out_dtype torch.float32, but out is torch.bfloat16"),
        ]
    for name, call in _blends(f16, bf16):                              # a mixture has no half type of its own: fp32 only
        rows += [
            (f"{name}: mixed features, fp16 out", lambda call=call: call(out=feat(f16)), TypeError, f"{name}: out is torch.float16; {f32_only}"),
            (f"{name}: mixed features, out_dtype bf16", lambda call=call: call(out_dtype=bf16), TypeError,
             f"{name}: out_dtype torch.bfloat16; expected torch.float32 (the features are not all of one half type)"),
        ]
    gm = lambda dt, **kw: merge.grain_merge(feat(dt, H // 4, W // 4), feat(dt, H // 2, W // 2), feat(dt), *masks(), **kw)
    gm_model = lambda dt, **kw: cgmodel.grain_merge(feat(dt, H // 4, W // 4), feat(dt, H // 2, W // 2), feat(dt), masks(), **kw)
    for side, call in (("merge", gm), ("model", gm_model)):
        rows += [
            (f"{side}.grain_merge: fp16 features, out_dtype bf16", lambda call=call: call(f16, out_dtype=bf16), TypeError,
             "grain_merge: out_dtype torch.bfloat16; expected torch.float32 or the features' torch.float16"),
            (f"{side}.grain_merge: fp32 features, out_dtype fp16", lambda call=call: call(f32, out_dtype=f16), TypeError,
             "grain_merge: out_dtype torch.float16; expected torch.float32 (the features are not all of one half type)"),
        ]
    rows += [
        ("merge.grain_merge: mixed features, out_dtype fp16",
         lambda: merge.grain_merge(feat(f16, H // 4, W // 4), feat(f32, H // 2, W // 2), feat(f16), *masks(), out_dtype=f16), TypeError,
         "grain_merge: out_dtype torch.float16; expected torch.float32 (the features are not all of one half type)"),
        ("merge.avg_pool: bf16 x, out_dtype fp16", lambda: merge.avg_pool(feat(bf16), 2, out_dtype=f16), TypeError,
         "avg_pool: out_dtype torch.float16; expected torch.float32 or the features' torch.bfloat16"),
        ("merge.avg_pool: fp32 x, out_dtype bf16", lambda: merge.avg_pool(feat(), 4, out_dtype=bf16), TypeError,
         "avg_pool: out_dtype torch.bfloat16; expected torch.float32 (the features are not all of one half type)"),
        ("merge.avg_pool: fp16 x, out_dtype int32", lambda: merge.avg_pool(feat(f16), 4, out_dtype=i32), TypeError,
         "avg_pool: out_dtype torch.int32; expected torch.float32 or the features' torch.float16"),
    ]
    return rows


ROWS = _rows()


@pytest.mark.parametrize("call, exc, message", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusal(call, exc, message):
    with FakeTensorMode():
        with pytest.raises(exc) as got:
            call()
    assert type(got.value) is exc
    assert got.value.args[0] == message


# ---------------------------------------------------------------------------- which entry point a call reaches
@pytest.fixture
def calls(monkeypatch):
    """the library call replaced by a recorder: [(entry point, arguments)], a tensor standing for its pointer"""
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(_lib, "ptr", lambda t: t)
    monkeypatch.setattr(_lib, "current_stream", lambda device=None: "stream")
    monkeypatch.setattr(_lib, "on_device", lambda device: _lib._null_ctx)
    return seen


def _four(dts, **kw):
    """the four operations on features of the types dts (cycled over an operation's features)"""
    d = lambda i: dts[i % len(dts)]
    mk = masks()
    return [merge.grain_merge(feat(d(0), H // 4, W // 4), feat(d(1), H // 2, W // 2), feat(d(2)), *mk, **kw),
            merge.avg_pool(feat(d(0)), 2, **kw),
            merge.decoder_blend_medium(feat(d(0), H // 2, W // 2), feat(d(1), H // 2, W // 2), mk[0], mk[1], BLEND_M, **kw),
            merge.decoder_blend_fine(feat(d(0)), feat(d(1)), *mk, **kw)]


def _tensors(args):
    return [a for a in args if isinstance(a, torch.Tensor)]


F32_CALLS = ["cgic_grain_merge_f32", "cgic_avgpool_f32", "cgic_decoder_blend_medium_f32", "cgic_decoder_blend_fine_f32"]
H_CALLS = ["cgic_grain_merge_h", "cgic_avgpool_h", "cgic_decoder_blend_medium_h", "cgic_decoder_blend_fine_h"]


@pytest.mark.parametrize("dts", [(f32,), (f16, bf16), (bf16, f16), (f16, f32), (f32, bf16), (f64,), (f16, f32, f16)],
                         ids=lambda d: "+".join(str(t).split(".")[1] for t in d))
def test_fp32_and_mixed_features_take_the_fp32_entry_points(calls, dts):
    """a mixture of feature types does not raise: every feature is cast to fp32, as every type was before ABI 16 (the pool has one
    feature and so no mixture: a half x is the half call's)"""
    with FakeTensorMode():
        outs = _four(dts)
    half_pool = dts[0] in (f16, bf16)
    assert [name for name, _ in calls] == [H_CALLS[1] if half_pool and i == 1 else n for i, n in enumerate(F32_CALLS)]
    for i, ((name, args), out) in enumerate(zip(calls, outs)):
        assert out.dtype == f32 and len(args) == len(_lib.PROTOTYPES[name][1])
        assert any(a is out for a in args)
        if not (half_pool and i == 1):
            assert all(t.dtype in (f32, i32) and t.is_contiguous() for t in _tensors(args))


@pytest.mark.parametrize("half", [f16, bf16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("to_half", [False, True], ids=["fp32-out", "half-out"])
def test_features_of_one_half_type_take_the_half_entry_points_without_a_cast(calls, half, to_half):
    with FakeTensorMode():
        outs = _four((half,), **({"out_dtype": half} if to_half else {}))
    assert [name for name, _ in calls] == H_CALLS
    code, res = merge._DT[half], half if to_half else f32
    for (name, args), out in zip(calls, outs):
        assert out.dtype == res and out.is_contiguous() and len(args) == len(_lib.PROTOTYPES[name][1])
        ts = _tensors(args)
        assert ts[-1] is out and all(t.dtype in (half, i32) for t in ts[:-1])          # the features as they came: no fp32 copy
        ints = [a for a in args if isinstance(a, int) and not isinstance(a, bool)]
        assert ints[0] == code and ints[-1] == merge._DT[res]                          # in_dtype first, out_dtype last


@pytest.mark.parametrize("half", [f16, bf16], ids=["fp16", "bf16"])
def test_out_decides_the_result_type_of_a_blend(calls, half):
    with FakeTensorMode():
        h, own, mk = feat(half), feat(half), masks()
        assert merge.decoder_blend_fine(h, own, *mk, out=h) is h                       # in place
        o32 = feat()
        assert cgmodel.decoder_blend_fine(h, own, mk, out=o32) is o32                  # the reference's promotion into a given buffer
        assert cgmodel.decoder_blend_medium(h, own, masks(2 * H, 2 * W)[:2], out=h, out_dtype=half) is h
        a = feat()
        assert cgmodel.decoder_blend_fine(a, feat(), mk, out=a) is a                   # fp32 as ever
    assert [name for name, _ in calls] == ["cgic_decoder_blend_fine_h", "cgic_decoder_blend_fine_h", "cgic_decoder_blend_medium_h",
                                           "cgic_decoder_blend_fine_f32"]
    out_codes = [[a for a in args if isinstance(a, int)][-1] for _, args in calls[:3]]
    assert out_codes == [merge._DT[half], 0, merge._DT[half]]
    assert calls[0][1][0] is calls[0][1][-3] and calls[1][1][-3] is o32               # (..., out, out_dtype, stream)


def test_avgpool_module_routes_half_inputs(calls, monkeypatch):
    """model.AvgPool: a 4-D device fp16 / bf16 input with H, W multiples of k goes to the half kernel and keeps its type unless
    autograd is needed; everything it did before stays"""
    fallback = []
    monkeypatch.setattr(torch.nn.functional, "avg_pool2d", lambda x, *a: fallback.append(x) or x)
    pool = cgmodel.AvgPool(2)
    with FakeTensorMode():
        x = feat(bf16)
        y = pool(x)
        assert y.dtype == bf16 and tuple(y.shape) == (B, C, H // 2, W // 2) and not fallback
        with torch.no_grad():
            assert pool(feat(f16).requires_grad_()).dtype == f16 and not fallback      # no autograd needed: the kernel
        xg = feat(f16).requires_grad_()
        assert pool(xg) is xg and len(fallback) == 1                                    # autograd needed: torch's pool
        assert pool(feat(bf16, h=H + 1)).shape[2] == H + 1 and len(fallback) == 2       # not a multiple of k: torch's pool, as before
        assert pool(feat(f64)).dtype == f64 and len(fallback) == 3
        assert pool(feat(bf16, device="cpu")).device.type == "cpu" and len(fallback) == 4
    assert [name for name, _ in calls] == ["cgic_avgpool_h", "cgic_avgpool_h"]
    assert calls[0][1][1] == 2 and calls[0][1][-2] == 2 and calls[1][1][1] == 1 and calls[1][1][-2] == 1


def test_nothing_new_is_exported_at_package_level():
    assert not [n for n in dir(cg) if n.endswith("_h") or "half" in n.lower()]
    assert cg.grain_merge is cgmodel.grain_merge and cg.decoder_blend_fine is cgmodel.decoder_blend_fine


# ---------------------------------------------------------------------------- the CPU statement that defines the pool's value
def pool_statement(x, k):
    """fp32 row-major running sum of every k x k window (starting from 0), divided by (float)(k*k), rounded once to x's type; a
    result of -0 -- a negative average that underflows the type -- is +0: ATen's kernel adds the rounded average onto a zeroed
    output element, and 0 + -0 is +0 (test_cpu_avg_pool2d_on_half_never_returns_minus_zero)"""
    xf = x.float()
    s = torch.zeros(x.shape[0], x.shape[1], x.shape[2] // k, x.shape[3] // k, dtype=f32)
    for dy in range(k):
        for dx in range(k):
            s = s + xf[:, :, dy::k, dx::k]
    r = (s / float(k * k)).to(x.dtype)
    return torch.where(r == 0, torch.zeros_like(r), r)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _special_finite(dtype):
    fi = torch.finfo(dtype)
    sub = [2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15] if dtype == f16 else [2.0 ** -133, 3 * 2.0 ** -133, 2.0 ** -127]      # subnormals of the type
    return [0.0, -0.0, fi.max, -fi.max, fi.max / 2, fi.tiny, -fi.tiny, fi.eps, 1.0, -1.0, 60000.0 if dtype == f16 else 3.0e38] + sub + [-v for v in sub]


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype", [f16, bf16], ids=["fp16", "bf16"])
def test_cpu_avg_pool2d_on_half_is_the_fp32_row_major_sum_rounded_once(dtype, k):
    gen = torch.Generator().manual_seed(100 * k + (dtype == f16))
    x = torch.randn(2, 3, 8 * k, 12 * k, generator=gen).to(dtype)
    x[0, 1] *= 1000.0                                                   # sums whose fp32 value needs more bits than the half type has
    x[1, 2] = (torch.randn(8 * k, 12 * k, generator=gen) * 2.0 ** -20).to(dtype)         # fp16: subnormal inputs and results
    win = lambda i, j: x[0, 0, i * k:(i + 1) * k, j * k:(j + 1) * k]
    sp = _special_finite(dtype)
    for n, v in enumerate(sp):                                          # every special value alone in a window of zeros, and filling one
        win(n // 12, n % 12)[:] = 0.0
        win(n // 12, n % 12)[0, 0] = v
        win(2 + n // 12, n % 12)[:] = v
    big = 60000.0 if dtype == f16 else 3.0e38
    win(4, 0)[:] = 0.0; win(4, 0)[0, 0] = big; win(4, 0)[0, 1] = big     # fp32 accumulation: 2 x 60000 averages to 30000 in fp16
    win(4, 1)[:] = big                                                   # a full window: the average is the value itself
    win(4, 2)[:] = torch.finfo(dtype).max                                # ... also at the largest finite value
    win(4, 3)[:] = 0.0; win(4, 3)[0, 0] = big; win(4, 3)[-1, -1] = -big
    assert torch.isfinite(x).all()
    got, want = torch.nn.functional.avg_pool2d(x, k, k, 0), pool_statement(x, k)
    assert got.dtype == dtype and not torch.isnan(got).any()          # (bf16: four of its largest values overflow the fp32 sum: +-Inf)
    if dtype == f16:
        assert float(got[0, 0, 4, 1]) == 60000.0 and float(got[0, 0, 4, 0]) == 2 * 60000.0 / (k * k) and float(got[0, 0, 4, 2]) == 65504.0
        assert bool(((got[1, 2] != 0) & (got[1, 2].abs() < 2.0 ** -14)).any())         # subnormal results are kept
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype", [f16, bf16], ids=["fp16", "bf16"])
def test_cpu_avg_pool2d_on_half_non_finite_inputs(dtype, k):
    """Inf and NaN anywhere in a window, and sums of finite values that overflow fp32 (bf16 only: fp16's largest value times 16
    fits): NaN in the same places, the same bits elsewhere"""
    x = torch.randn(1, 2, 4 * k, 6 * k, generator=torch.Generator().manual_seed(k)).to(dtype)
    win = lambda i, j: x[0, 0, i * k:(i + 1) * k, j * k:(j + 1) * k]
    win(0, 0)[0, 0] = np.inf
    win(0, 1)[-1, -1] = -np.inf
    win(0, 2)[0, 0] = np.inf; win(0, 2)[-1, -1] = -np.inf                # Inf - Inf
    win(0, 3)[0, 1] = np.nan
    win(1, 0)[:] = np.inf
    win(1, 1)[:] = np.nan
    win(1, 2)[:] = torch.finfo(dtype).max                                # bf16: the fp32 sum overflows after two terms
    win(1, 3)[:] = -torch.finfo(dtype).max
    got, want = torch.nn.functional.avg_pool2d(x, k, k, 0), pool_statement(x, k)
    assert torch.isnan(want[0, 0, 0, 2]) and torch.isnan(want[0, 0, 0, 3]) and want[0, 0, 0, 0] == np.inf and want[0, 0, 0, 1] == -np.inf
    assert want[0, 0, 1, 2] == (np.inf if dtype == bf16 else 65504.0)
    assert np.array_equal(torch.isnan(got).numpy(), torch.isnan(want).numpy())
    keep = ~torch.isnan(want)
    assert np.array_equal(_bits(got[keep]), _bits(want[keep]))


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype,e", [(f16, -24), (bf16, -133)], ids=["fp16", "bf16"])
def test_cpu_avg_pool2d_on_half_never_returns_minus_zero(dtype, e, k):
    """windows of small multiples of the type's smallest subnormal 2^e: wherever the rounded average is -0 (the fp32 average is
    negative and at most half that subnormal in size) ATen's kernel returns +0, and it equals the rounded average everywhere else.
    The half pool kernel stores +0 there too; a window of -0 alone is +0 either way (0 + -0)."""
    x = (torch.randint(-6, 7, (4, 8, 16 * k, 16 * k), generator=torch.Generator().manual_seed(k)).float() * 2.0 ** e).to(dtype)
    x[0, 0, :k, :k] = -0.0
    xf = x.float()
    s = torch.zeros(4, 8, 16, 16)
    for dy in range(k):
        for dx in range(k):
            s = s + xf[:, :, dy::k, dx::k]
    rounded = (s / float(k * k)).to(dtype)
    minus_zero = torch.from_numpy(_bits(rounded) == -32768)
    assert int(minus_zero.sum()) > 100 and bool((s[minus_zero] < 0).all())
    got = torch.nn.functional.avg_pool2d(x, k, k, 0)
    assert not (_bits(got) == -32768).any() and bool((_bits(got)[minus_zero.numpy()] == 0).all())
    assert np.array_equal(_bits(got)[~minus_zero.numpy()], _bits(rounded)[~minus_zero.numpy()])
    assert np.array_equal(_bits(got), _bits(pool_statement(x, k)))
