"""CPU: the SpatialNorm path (ABI 17) as far as it goes without a device.

  - the shape of the ABI: the three entry points in the header, the library and the ctypes table;
  - what norm.spatial_norm refuses, with the full message, under FakeTensorMode on fake "cuda" tensors (every check sits in front of
    the first data_ptr(), `out=` included);
  - which inputs reach the kernel and which reach torch (SpatialNorm.uses_kernel), and that the torch path is the reference's
    expression;
  - adopt() keeps the parameter objects and the state_dict keys of the real class (recorded in the fixture); install()'s default
    leaves the norms alone;
  - the float64 restatement that the GPU tests measure against (tests/spatial_norm_ref.py) is held to tests/golden/spatial_norm.npz,
    which tests/golden/make_golden_norm.py wrote from the real class; torch's fp32 evaluation errs as the class's own did.
"""
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib, norm
import spatial_norm_ref as ref

f32, f16, bf16, f64, i32 = torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgic_spatial_norm": 23, "cgic_spatial_norm_workspace_bytes": 6, "cgic_spatial_norm_one_launch": 6}
CASES = ("up2", "up4_up2", "same", "down4", "down4_up2")
B, C, H, W = 2, 64, 8, 12
CPU_TENSOR = ("control_gic_amd ops run on an MI355X (HIP) device only; got a CPU tensor. "
              "There is deliberately no CPU fallback -- the CPU oracle lives in oracle/ and is test-only.")


# ---------------------------------------------------------------------------- the ABI
def test_abi_17_declares_exports_and_binds_the_three_entry_points():
    assert _lib.lib().cgic_abi_version() >= 17
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgic_hip.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        args = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr).group(1)
        assert len(args.split(",")) == nargs, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert norm._DT == {f32: 0, f16: 1, bf16: 2}
    assert {"norm", "SpatialNorm", "spatial_norm"} <= set(cg.__all__)
    assert str(torch.ops.cgic.spatial_norm.default._schema) == (
        "cgic::spatial_norm(Tensor f, Tensor zq, Tensor gn_weight, Tensor gn_bias, Tensor wy, Tensor by, Tensor wb, Tensor bb, "
        "SymInt groups, float eps, bool swish, bool half_out) -> Tensor")


# ---------------------------------------------------------------------------- refusals (FakeTensorMode)
def T(*shape, dtype=f32, device="cuda"):
    return torch.empty(shape, dtype=dtype, device=device)


def args(dtype=f32, hq=4, wq=6, **over):
    a = dict(f=T(B, C, H, W, dtype=dtype), zq=T(B, 4, hq, wq), gn_w=T(C), gn_b=T(C), wy=T(C, 4, 1, 1), by=T(C), wb=T(C, 4, 1, 1), bb=T(C))
    a.update(over)
    return [a[k] for k in ref.ORDER]


ROWS = [
    ("cpu features", lambda: norm.spatial_norm(*args(f=T(B, C, H, W, device="cpu"))), RuntimeError, CPU_TENSOR),
    ("cpu zq", lambda: norm.spatial_norm(*args(zq=T(B, 4, 4, 6, device="cpu"))), RuntimeError, CPU_TENSOR),
    ("cpu parameter", lambda: norm.spatial_norm(*args(wb=T(C, 4, device="cpu"))), RuntimeError, CPU_TENSOR),
    ("cpu out", lambda: norm.spatial_norm(*args(), out=T(B, C, H, W, device="cpu")), RuntimeError, CPU_TENSOR),
    ("fp64 features", lambda: norm.spatial_norm(*args(f=T(B, C, H, W, dtype=f64))), TypeError,
     f"spatial_norm: features torch.float64 {(B, C, H, W)}; expected fp32, fp16 or bf16 [B,C,H,W]"),
    ("3-d features", lambda: norm.spatial_norm(*args(f=T(C, H, W))), TypeError,
     f"spatial_norm: features torch.float32 {(C, H, W)}; expected fp32, fp16 or bf16 [B,C,H,W]"),
    ("groups", lambda: norm.spatial_norm(*args(), groups=48), ValueError, "spatial_norm: 64 channels in 48 groups"),
    ("zq channels", lambda: norm.spatial_norm(*args(zq=T(B, 3, 4, 6))), ValueError,
     f"spatial_norm: zq torch.float32 {(B, 3, 4, 6)}; expected [{B},4,hq,wq]"),
    ("zq batch", lambda: norm.spatial_norm(*args(zq=T(B + 1, 4, 4, 6))), ValueError,
     f"spatial_norm: zq torch.float32 {(B + 1, 4, 4, 6)}; expected [{B},4,hq,wq]"),
    ("int zq", lambda: norm.spatial_norm(*args(zq=T(B, 4, 4, 6, dtype=i32))), ValueError,
     f"spatial_norm: zq torch.int32 {(B, 4, 4, 6)}; expected [{B},4,hq,wq]"),
    ("ratio y", lambda: norm.spatial_norm(*args(hq=3)), ValueError,
     "spatial_norm: zq 3x6 under features 8x12: each axis must be an integer ratio, up or down"),
    ("ratio x", lambda: norm.spatial_norm(*args(wq=8)), ValueError,
     "spatial_norm: zq 4x8 under features 8x12: each axis must be an integer ratio, up or down"),
    ("gn_weight of another length", lambda: norm.spatial_norm(*args(gn_w=T(C + 1))), ValueError,
     f"spatial_norm: gn_weight torch.float32 {(C + 1,)}; expected {C} floating-point values"),
    ("wy transposed", lambda: norm.spatial_norm(*args(wy=T(4, C))), ValueError,
     f"spatial_norm: wy torch.float32 {(4, C)}; expected {4 * C} floating-point values as [{C},4]"),
    ("int bias", lambda: norm.spatial_norm(*args(bb=T(C, dtype=i32))), ValueError,
     f"spatial_norm: bb torch.int32 {(C,)}; expected {C} floating-point values"),
    ("out of another shape", lambda: norm.spatial_norm(*args(), out=T(B, C, H, W - 4)), ValueError,
     f"spatial_norm: out {(B, C, H, W - 4)} must have f's shape {(B, C, H, W)}"),
    ("out not contiguous", lambda: norm.spatial_norm(*args(), out=T(B, C, W, H).transpose(2, 3)), ValueError, "spatial_norm: out must be contiguous"),
    ("fp32 features, fp16 out", lambda: norm.spatial_norm(*args(), out=T(B, C, H, W, dtype=f16)), TypeError,
     "spatial_norm: out is torch.float16; the result of these features is torch.float32"),
    ("fp16 features, bf16 out", lambda: norm.spatial_norm(*args(f16), out=T(B, C, H, W, dtype=bf16)), TypeError,
     "spatial_norm: out is torch.bfloat16; expected torch.float32 or the features' torch.float16"),
    ("out_dtype against out", lambda: norm.spatial_norm(*args(f16), out=T(B, C, H, W, dtype=f16), out_dtype=f32), TypeError,
     "spatial_norm: out_dtype torch.float32, but out is torch.float16"),
    ("fp32 features, fp16 out_dtype", lambda: norm.spatial_norm(*args(), out_dtype=f16), TypeError,
     "spatial_norm: out_dtype torch.float16; expected torch.float32"),
    ("bf16 features, fp16 out_dtype", lambda: norm.spatial_norm(*args(bf16), out_dtype=f16), TypeError,
     "spatial_norm: out_dtype torch.float16; expected torch.float32 or the features' torch.bfloat16"),
    ("the op, cpu features", lambda: norm.spatial_norm_op._init_fn(*args(f=T(B, C, H, W, device="cpu")), 32, 1e-6, False, False), RuntimeError, CPU_TENSOR),
    ("the op, ratio", lambda: norm.spatial_norm_op._init_fn(*args(hq=5), 32, 1e-6, False, False), ValueError,
     "spatial_norm: zq 5x6 under features 8x12: each axis must be an integer ratio, up or down"),
]


@pytest.mark.parametrize("call, exc, text", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusals_come_before_the_first_data_ptr(call, exc, text):
    with FakeTensorMode():
        with pytest.raises(exc) as got:
            call()
    assert str(got.value) == text


def test_the_fake_kernel_gives_shape_and_dtype():
    with FakeTensorMode():
        for dtype, half_out, want in ((f32, False, f32), (f32, True, f32), (f16, False, f32), (f16, True, f16), (bf16, True, bf16)):
            out = torch.ops.cgic.spatial_norm(*args(dtype), 32, 1e-6, True, half_out)
            assert tuple(out.shape) == (B, C, H, W) and out.dtype == want and out.device.type == "cuda"


# ---------------------------------------------------------------------------- the module
def test_adopt_keeps_parameters_and_the_reference_state_dict_keys(golden):
    g = golden("spatial_norm")
    for name, add_conv in (("up2", False), ("add_conv", True)):
        theirs = ref.StandIn(32, 4, add_conv=add_conv)
        mine = norm.SpatialNorm.adopt(theirs)
        assert list(mine.state_dict().keys()) == [str(k) for k in g[name + "/keys"]]
        assert all(p is q for p, q in zip(mine.parameters(), theirs.parameters()))
        assert mine.norm_layer is theirs.norm_layer and mine.conv_y is theirs.conv_y and mine.conv_b is theirs.conv_b
        own = norm.SpatialNorm(32, 4, add_conv=add_conv, num_groups=32, eps=1e-6, affine=True)        # the reference's constructor
        assert list(own.state_dict().keys()) == list(mine.state_dict().keys())
        assert own.norm_layer.num_groups == 32 and own.norm_layer.eps == 1e-6
        own.load_state_dict(theirs.state_dict())
    frozen = norm.SpatialNorm(32, 4, freeze_norm_layer=True, num_groups=32)
    assert not any(p.requires_grad for p in frozen.norm_layer.parameters()) and frozen.conv_y.weight.requires_grad
    with pytest.raises(TypeError, match="SpatialNorm.adopt: GroupNorm has not the reference's"):
        norm.SpatialNorm.adopt(torch.nn.GroupNorm(32, 64))
    three = ref.StandIn(32)
    three.conv_y = torch.nn.Conv2d(4, 32, 3, padding=1)
    assert not norm.has_reference_shape(three) and norm.has_reference_shape(ref.StandIn(32))


def test_which_inputs_reach_the_kernel_and_which_reach_torch():
    m = norm.SpatialNorm.adopt(ref.StandIn(C)).eval()
    with FakeTensorMode():
        f, zq = T(B, C, H, W), T(B, 4, 4, 6)
        with torch.no_grad():
            assert m.uses_kernel(f, zq)
            assert m.uses_kernel(T(B, C, H, W, dtype=f16), zq) and m.uses_kernel(T(B, C, H, W, dtype=bf16), T(B, 4, 16, 24))
            assert not m.uses_kernel(T(B, C, H, W, device="cpu"), T(B, 4, 4, 6, device="cpu"))
            assert not m.uses_kernel(f, T(B, 4, 4, 6, device="cpu"))
            assert not m.uses_kernel(f, T(B, 4, 3, 6)) and not m.uses_kernel(f, T(B, 4, 4, 5))          # no integer ratio
            assert not m.uses_kernel(f, T(B, 3, 4, 6))                                                 # zq channels
            assert not m.uses_kernel(T(B, C, H, W, dtype=f64), zq)
        assert not m.uses_kernel(f, zq)                     # the parameters want a gradient and autograd is on
        for p in m.parameters():
            p.requires_grad_(False)
        assert m.uses_kernel(f, zq)
        assert not m.uses_kernel(T(B, C, H, W).requires_grad_(), zq)
    other = ref.StandIn(C)
    other.norm_layer = torch.nn.BatchNorm2d(C)
    plain = ref.StandIn(C)
    plain.norm_layer = torch.nn.GroupNorm(32, C, affine=False)
    five = ref.StandIn(C, zq_channels=5)
    with FakeTensorMode(), torch.no_grad():
        assert not norm.SpatialNorm.adopt(other).uses_kernel(T(B, C, H, W), T(B, 4, 4, 6))
        assert not norm.SpatialNorm.adopt(plain).uses_kernel(T(B, C, H, W), T(B, 4, 4, 6))
        assert not norm.SpatialNorm.adopt(five).uses_kernel(T(B, C, H, W), T(B, 5, 4, 6))
        # add_conv: torch interpolates and convolves, then the kernel runs at ratio 1 -- any size of zq will do
        assert norm.SpatialNorm.adopt(ref.StandIn(C, add_conv=True)).uses_kernel(T(B, C, H, W), T(B, 4, 3, 5))


@pytest.mark.parametrize("name", CASES + ("add_conv",))
def test_the_torch_path_is_the_reference(golden, name):
    """on the CPU the module evaluates the reference's expression: the recorded float64 result of the real class, to float64 rounding"""
    g = golden("spatial_norm")
    _, Cc, _, _, _, _, add_conv = (int(v) for v in g[name + "/shape"])
    m = norm.SpatialNorm(Cc, 4, add_conv=bool(add_conv), num_groups=32, eps=1e-6, affine=True)
    m.load_state_dict({str(k): torch.from_numpy(g[f"{name}/{k}"]) for k in g[name + "/keys"]})
    m = m.double().eval()
    f, zq = torch.from_numpy(g[name + "/f"]).double(), torch.from_numpy(g[name + "/zq"]).double()
    want = torch.from_numpy(g[name + "/ref64"])
    with torch.no_grad():
        assert not m.uses_kernel(f, zq)
        assert float((m(f, zq) - want).abs().max()) < 1e-12
        sw = m(f, zq, swish=True)
        assert float((sw - want * torch.sigmoid(want)).abs().max()) < 1e-12 and m(f, zq, out_dtype=f32).dtype == f32


def test_default_install_leaves_the_norms_alone():
    import inspect
    sig = inspect.signature(cg.install)
    assert sig.parameters["patch_norms"].default is False and sig.parameters["patch_pools"].default is True
    holder = torch.nn.Module()
    holder.a, holder.b = ref.StandIn(32), torch.nn.Sequential(ref.StandIn(64, add_conv=True), torch.nn.GroupNorm(32, 64))
    assert norm.patch_norms(holder) == 2 and norm.patch_norms(holder) == 0
    assert type(holder.a) is norm.SpatialNorm and type(holder.b[0]) is norm.SpatialNorm and type(holder.b[1]) is torch.nn.GroupNorm


# ---------------------------------------------------------------------------- the restatement, held to the fixture
@pytest.mark.parametrize("name", CASES)
def test_the_restatement_is_the_real_class(golden, name):
    g = golden("spatial_norm")
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"])
    a = (t("f"), t("zq"), t("norm_layer.weight"), t("norm_layer.bias"), t("conv_y.weight"), t("conv_y.bias"), t("conv_b.weight"), t("conv_b.bias"))
    want = t("ref64")
    assert want.dtype == f64
    assert float((ref.restatement(*a) - want).abs().max()) < 1e-12
    assert float((ref.restatement(*a, swish=True) - want * torch.sigmoid(want)).abs().max()) < 1e-12
    # E_ref, the unit of the GPU tests' bar: torch's fp32 ops err as the real class's own fp32 run did when the fixture was written
    # (the same ops; a factor of 2 for another build of torch)
    e = ref.e_ref(want, *a)
    recorded = float(g[name + "/err32"])
    assert 0 < e <= 2 * recorded and recorded <= 2 * e and recorded < 1e-5


def test_the_closed_form_of_the_nearest_index_is_torchs():
    for n, nq in ((8, 2), (6, 6), (6, 24), (16, 64), (12, 3), (2, 8), (5, 5), (9, 3)):
        want = torch.nn.functional.interpolate(torch.arange(nq, dtype=f64).reshape(1, 1, nq, 1), size=(n, 1), mode="nearest").reshape(-1)
        assert ref.nearest(n, nq).tolist() == want.long().tolist() == norm.nearest_index(n, nq)
    assert not norm.integer_ratio(6, 4) and not norm.integer_ratio(4, 6) and norm.integer_ratio(4, 4)
    with pytest.raises(ValueError, match="4 rows of zq under 6 of the features is not an integer ratio"):
        norm.nearest_index(6, 4)
