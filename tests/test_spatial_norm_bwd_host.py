"""CPU: SpatialNorm for training (ABI 19) as far as it goes without a device.

  - the shape of the ABI: the three entry points in the header, the library and the ctypes table; the op's schema;
  - what norm.spatial_norm_train / spatial_norm_backward refuse, with the full message, under FakeTensorMode on fake "cuda" tensors
    (every check sits in front of the first data_ptr());
  - the fake kernel of torch.ops.cgic.spatial_norm_train gives shapes and dtypes;
  - SpatialNorm.backward_kernel defaults off (adopt() included); with it off, uses_kernel and the module's behaviour are what they
    were; with it on, which calls reach the training kernels;
  - the differentiable float64 restatement that the GPU tests measure against (tests/spatial_norm_bwd_ref.py) is held to
    tests/golden/spatial_norm_bwd.npz, the gradients that tests/golden/make_golden_norm_bwd.py recorded from the real class;
  - E_ref, the unit of the GPU tests' bar, is positive and finite for every gradient on every shape of those tests.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib, norm
import spatial_norm_ref as ref
import spatial_norm_bwd_ref as bref

f32, f16, bf16, f64, i32 = torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgic_spatial_norm_train": 24, "cgic_spatial_norm_backward": 32, "cgic_spatial_norm_backward_workspace_bytes": 6}
B, C, H, W = 2, 64, 8, 12
CPU_TENSOR = ("control_gic_amd ops run on an MI355X (HIP) device only; got a CPU tensor. "
              "There is deliberately no CPU fallback -- the CPU oracle lives in oracle/ and is test-only.")
# the shapes of tests/test_spatial_norm_bwd.py: C, H, W, hq, wq
SHAPES = [(32, 2, 2, 2, 2), (32, 3, 5, 3, 5), (32, 4, 6, 2, 3), (64, 6, 10, 24, 40), (64, 6, 10, 12, 5), (32, 34, 68, 17, 17), (512, 16, 16, 64, 64)]


# ---------------------------------------------------------------------------- the ABI
def test_abi_19_declares_exports_and_binds_the_three_entry_points():
    assert _lib.lib().cgic_abi_version() >= 19
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgic_hip.h")).read(), flags=re.S)
    assert int(re.search(r"^#define\s+CGIC_ABI_VERSION\s+(\d+)", hdr, re.M).group(1)) >= 19
    for name, nargs in NEW.items():
        args = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr).group(1)
        assert len(args.split(",")) == nargs, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert norm.GRADS == ("f", "zq", "gn_weight", "gn_bias", "wy", "by", "wb", "bb")
    assert str(torch.ops.cgic.spatial_norm_train.default._schema) == (
        "cgic::spatial_norm_train(Tensor f, Tensor zq, Tensor gn_weight, Tensor gn_bias, Tensor wy, Tensor by, Tensor wb, Tensor bb, "
        "SymInt groups, float eps, bool swish, bool half_out) -> (Tensor, Tensor)")
    assert str(torch.ops.cgic.spatial_norm.default._schema).endswith("bool half_out) -> Tensor")          # the inference op stays


# ---------------------------------------------------------------------------- refusals (FakeTensorMode)
def T(*shape, dtype=f32, device="cuda"):
    return torch.empty(shape, dtype=dtype, device=device)


def args(dtype=f32, hq=4, wq=6, **over):
    a = dict(f=T(B, C, H, W, dtype=dtype), zq=T(B, 4, hq, wq), gn_w=T(C), gn_b=T(C), wy=T(C, 4, 1, 1), by=T(C), wb=T(C, 4, 1, 1), bb=T(C))
    a.update(over)
    return [a[k] for k in ref.ORDER]


def bwd(dtype=f32, go=None, stats=None, **over):
    """the arguments of spatial_norm_backward: go, f, zq, stats, the six parameters"""
    kw = {k: over.pop(k) for k in ("need", "df_dtype", "outs", "workspace", "groups") if k in over}
    a = args(dtype, **over)
    go = T(B, C, H, W, dtype=dtype) if go is None else go
    stats = T(B * 32, 2) if stats is None else stats
    return norm.spatial_norm_backward(go, a[0], a[1], stats, *a[2:], **kw)


N = "spatial_norm_backward"
ROWS = [
    ("train: cpu features", lambda: norm.spatial_norm_train(*args(f=T(B, C, H, W, device="cpu"))), RuntimeError, CPU_TENSOR),
    ("train: fp64 features", lambda: norm.spatial_norm_train(*args(f=T(B, C, H, W, dtype=f64))), TypeError,
     f"spatial_norm_train: features torch.float64 {(B, C, H, W)}; expected fp32, fp16 or bf16 [B,C,H,W]"),
    ("train: groups", lambda: norm.spatial_norm_train(*args(), groups=48), ValueError, "spatial_norm_train: 64 channels in 48 groups"),
    ("train: ratio", lambda: norm.spatial_norm_train(*args(hq=3)), ValueError,
     "spatial_norm_train: zq 3x6 under features 8x12: each axis must be an integer ratio, up or down"),
    ("train: wy transposed", lambda: norm.spatial_norm_train(*args(wy=T(4, C))), ValueError,
     f"spatial_norm_train: wy torch.float32 {(4, C)}; expected {4 * C} floating-point values as [{C},4]"),
    ("train: out of another shape", lambda: norm.spatial_norm_train(*args(), out=T(B, C, H, W - 4)), ValueError,
     f"spatial_norm_train: out {(B, C, H, W - 4)} must have f's shape {(B, C, H, W)}"),
    ("train: fp32 features, fp16 out_dtype", lambda: norm.spatial_norm_train(*args(), out_dtype=f16), TypeError,
     "spatial_norm_train: out_dtype torch.float16; expected torch.float32"),
    ("the op, ratio", lambda: norm.spatial_norm_train_op._init_fn(*args(hq=5), 32, 1e-6, False, False), ValueError,
     "spatial_norm_train: zq 5x6 under features 8x12: each axis must be an integer ratio, up or down"),
    ("cpu go", lambda: bwd(go=T(B, C, H, W, device="cpu")), RuntimeError, CPU_TENSOR),
    ("cpu stats", lambda: bwd(stats=T(B * 32, 2, device="cpu")), RuntimeError, CPU_TENSOR),
    ("cpu workspace", lambda: bwd(workspace=T(1 << 20, dtype=torch.uint8, device="cpu")), RuntimeError, CPU_TENSOR),
    ("cpu outs", lambda: bwd(outs={"by": T(C, device="cpu")}), RuntimeError, CPU_TENSOR),
    ("fp64 features", lambda: bwd(f=T(B, C, H, W, dtype=f64)), TypeError, f"{N}: features torch.float64 {(B, C, H, W)}; expected fp32, fp16 or bf16 [B,C,H,W]"),
    ("groups", lambda: bwd(groups=48), ValueError, f"{N}: 64 channels in 48 groups"),
    ("ratio x", lambda: bwd(wq=8), ValueError, f"{N}: zq 4x8 under features 8x12: each axis must be an integer ratio, up or down"),
    ("int bias", lambda: bwd(bb=T(C, dtype=i32)), ValueError, f"{N}: bb torch.int32 {(C,)}; expected {C} floating-point values"),
    ("need nothing", lambda: bwd(need=()), ValueError, f"{N}: need (), outs (); expected names out of {norm.GRADS}, at least one, outs among the needed"),
    ("need an unknown name", lambda: bwd(need=("f", "gamma")), ValueError,
     f"{N}: need ('f', 'gamma'), outs (); expected names out of {norm.GRADS}, at least one, outs among the needed"),
    ("outs that are not needed", lambda: bwd(need=("f",), outs={"by": T(C)}), ValueError,
     f"{N}: need ('f',), outs ('by',); expected names out of {norm.GRADS}, at least one, outs among the needed"),
    ("empty batch", lambda: norm.spatial_norm_backward(T(0, C, H, W), T(0, C, H, W), T(0, 4, 4, 6), T(0, 2), *args()[2:]), ValueError, f"{N}: an empty batch"),
    ("go of another shape", lambda: bwd(go=T(B, C, H, W + 1)), TypeError, f"{N}: go torch.float32 {(B, C, H, W + 1)}; expected {(B, C, H, W)} in torch.float32"),
    ("fp16 go on fp32 features", lambda: bwd(go=T(B, C, H, W, dtype=f16)), TypeError,
     f"{N}: go torch.float16 {(B, C, H, W)}; expected {(B, C, H, W)} in torch.float32"),
    ("bf16 go on fp16 features", lambda: bwd(f16, go=T(B, C, H, W, dtype=bf16)), TypeError,
     f"{N}: go torch.bfloat16 {(B, C, H, W)}; expected {(B, C, H, W)} in torch.float32 or torch.float16"),
    ("stats of another shape", lambda: bwd(stats=T(B * 32)), TypeError, f"{N}: stats torch.float32 {(B * 32,)}; expected torch.float32 [{B * 32}, 2] (spatial_norm_train's)"),
    ("fp16 stats", lambda: bwd(stats=T(B * 32, 2, dtype=f16)), TypeError, f"{N}: stats torch.float16 {(B * 32, 2)}; expected torch.float32 [{B * 32}, 2] (spatial_norm_train's)"),
    ("fp16 df of fp32 features", lambda: bwd(df_dtype=f16), TypeError, f"{N}: df_dtype torch.float16; expected torch.float32"),
    ("bf16 df of fp16 features", lambda: bwd(f16, df_dtype=bf16), TypeError, f"{N}: df_dtype torch.bfloat16; expected torch.float32 or the features' torch.float16"),
    ("outs of another shape", lambda: bwd(outs={"wy": T(C, 4)}), ValueError,
     f"{N}: outs['wy'] torch.float32 {(C, 4)} on cuda:0; expected contiguous torch.float32 {(C, 4, 1, 1)} on cuda:0"),
    ("half dzq", lambda: bwd(outs={"zq": T(B, 4, 4, 6, dtype=f16)}), ValueError,
     f"{N}: outs['zq'] torch.float16 {(B, 4, 4, 6)} on cuda:0; expected contiguous torch.float32 {(B, 4, 4, 6)} on cuda:0"),
    ("a short workspace", lambda: bwd(workspace=T(100, dtype=torch.uint8)), ValueError,
     f"{N}: workspace torch.uint8 of 100 elements; expected contiguous torch.uint8 of at least "
     f"{B * C * 96 + B * C * 16 + B * 8 * 4 * H * W * 4} on cuda:0"),
]


@pytest.mark.parametrize("call, exc, text", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusals_come_before_the_first_data_ptr(call, exc, text):
    with FakeTensorMode():
        with pytest.raises(exc) as got:
            call()
    assert str(got.value) == text


def test_the_fake_kernel_gives_shapes_and_dtypes():
    with FakeTensorMode():
        for dtype, half_out, want in ((f32, False, f32), (f32, True, f32), (f16, False, f32), (f16, True, f16), (bf16, True, bf16)):
            out, stats = torch.ops.cgic.spatial_norm_train(*args(dtype), 32, 1e-6, True, half_out)
            assert tuple(out.shape) == (B, C, H, W) and out.dtype == want and out.device.type == "cuda"
            assert tuple(stats.shape) == (B * 32, 2) and stats.dtype == f32 and stats.device.type == "cuda"
        out, stats = torch.ops.cgic.spatial_norm_train(*args(), 16, 1e-6, False, False)
        assert tuple(stats.shape) == (B * 16, 2)


def test_the_op_is_differentiable_in_its_ten_tensors_under_fake_tensors():
    """the autograd formula is registered: the output of the op carries a grad_fn when an input wants a gradient"""
    with FakeTensorMode():
        a = args()
        a[0].requires_grad_()
        out, stats = torch.ops.cgic.spatial_norm_train(*a, 32, 1e-6, True, False)
        assert out.requires_grad and out.grad_fn is not None
        with torch.no_grad():
            out, _ = torch.ops.cgic.spatial_norm_train(*a, 32, 1e-6, True, False)
        assert not out.requires_grad


# ---------------------------------------------------------------------------- the module and install()
def test_the_flag_defaults_off_and_off_is_todays_behaviour():
    assert norm.SpatialNorm.backward_kernel is False
    own = norm.SpatialNorm(C, 4, num_groups=32, eps=1e-6, affine=True)
    adopted = norm.SpatialNorm.adopt(ref.StandIn(C))                            # (adopt() bypasses __init__)
    assert own.backward_kernel is False and adopted.backward_kernel is False and "backward_kernel" not in vars(adopted)
    assert inspect.signature(cg.install).parameters["norm_backward"].default is False
    assert inspect.signature(cg.install).parameters["patch_norms"].default is False
    assert inspect.signature(norm.patch_norms).parameters["backward_kernel"].default is False
    m = adopted.eval()
    with FakeTensorMode():
        f, zq = T(B, C, H, W), T(B, 4, 4, 6)
        assert not m.uses_kernel(f, zq) and not m.uses_backward_kernel(f, zq)   # the parameters want a gradient: torch's path
        with torch.no_grad():
            assert m.uses_kernel(f, zq) and not m.uses_backward_kernel(f, zq)
    # on the CPU, with autograd, the module is the reference's expression bit for bit, flag or no flag
    theirs = ref.randomize(ref.StandIn(32), 3)
    mine = norm.SpatialNorm.adopt(theirs)
    rng = np.random.default_rng(1)
    f = torch.from_numpy(rng.standard_normal((2, 32, 4, 6)).astype(np.float32)).requires_grad_()
    zq = torch.from_numpy(rng.standard_normal((2, 4, 2, 3)).astype(np.float32))
    for flag in (False, True):
        mine.backward_kernel = flag
        assert not mine.uses_backward_kernel(f, zq)                              # CPU tensors never reach a kernel
        got, want = mine(f, zq), theirs(f, zq)
        assert torch.equal(got, want)
        assert torch.equal(torch.autograd.grad(got.sum(), f)[0], torch.autograd.grad(want.sum(), f)[0])


def test_with_the_flag_on_the_calls_that_need_a_gradient_reach_the_training_kernels():
    m = norm.SpatialNorm.adopt(ref.StandIn(C)).eval()
    m.backward_kernel = True
    with FakeTensorMode(allow_non_fake_inputs=True):             # (the module's parameters are real tensors)
        f, zq = T(B, C, H, W), T(B, 4, 4, 6)
        assert m.uses_backward_kernel(f, zq) and not m.uses_kernel(f, zq)
        assert m.uses_backward_kernel(T(B, C, H, W, dtype=f16), zq) and m.uses_backward_kernel(T(B, C, H, W, dtype=bf16), T(B, 4, 16, 24))
        out = m(f, zq, swish=True)
        assert out.grad_fn is not None and out.dtype == f32 and tuple(out.shape) == (B, C, H, W)
        assert m(T(B, C, H, W, dtype=f16), zq, out_dtype=f16).dtype == f16
        with torch.no_grad():                                   # nothing needs a gradient: the inference kernel, as before
            assert m.uses_kernel(f, zq) and not m.uses_backward_kernel(f, zq)
        # what the kernels do not serve stays on torch's path
        assert not m.uses_backward_kernel(f, T(B, 4, 3, 6)) and not m.uses_backward_kernel(f, T(B, 3, 4, 6))
        assert not m.uses_backward_kernel(T(B, C, H, W, device="cpu"), T(B, 4, 4, 6, device="cpu"))
        assert not m.uses_backward_kernel(T(B, C, H, W, dtype=f64), zq)
        assert not m.uses_backward_kernel(T(0, C, H, W), T(0, 4, 4, 6)) and not m.uses_kernel(T(0, C, H, W), T(0, 4, 4, 6))     # an empty batch: torch's path
        for p in m.parameters():
            p.requires_grad_(False)
        assert m.uses_kernel(f, zq) and not m.uses_backward_kernel(f, zq)
        assert m.uses_backward_kernel(T(B, C, H, W).requires_grad_(), zq)       # frozen parameters, features that want a gradient
        plain = ref.StandIn(C)
        plain.norm_layer = torch.nn.GroupNorm(32, C, affine=False)
        p = norm.SpatialNorm.adopt(plain)
        p.backward_kernel = True
        assert not p.uses_backward_kernel(T(B, C, H, W).requires_grad_(), zq)
        ac = norm.SpatialNorm.adopt(ref.StandIn(C, add_conv=True))
        ac.backward_kernel = True
        assert ac.uses_backward_kernel(T(B, C, H, W), T(B, 4, 3, 5))            # add_conv: torch interpolates and convolves first


def test_patch_norms_sets_the_flag_only_when_asked():
    holder = torch.nn.Module()
    holder.a, holder.b = ref.StandIn(32), torch.nn.Sequential(ref.StandIn(64, add_conv=True), torch.nn.GroupNorm(32, 64))
    assert norm.patch_norms(holder) == 2
    assert holder.a.backward_kernel is False and holder.b[0].backward_kernel is False
    assert norm.patch_norms(holder, backward_kernel=True) == 0                  # nothing left to swap; the flag reaches those swapped before
    assert holder.a.backward_kernel is True and holder.b[0].backward_kernel is True
    assert norm.SpatialNorm.backward_kernel is False                             # the class is untouched
    fresh = torch.nn.Module()
    fresh.n = ref.StandIn(32)
    assert norm.patch_norms(fresh, backward_kernel=True) == 1 and fresh.n.backward_kernel is True


# ---------------------------------------------------------------------------- the restatement, held to the fixture
@pytest.mark.parametrize("swish", [False, True])
def test_the_restatements_gradients_are_the_real_classs(golden, swish):
    g = golden("spatial_norm_bwd")
    name = "up2_down2"
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"])
    x = dict(f=t("f"), zq=t("zq"), gn_w=t("norm_layer.weight"), gn_b=t("norm_layer.bias"), wy=t("conv_y.weight"), by=t("conv_y.bias"),
             wb=t("conv_b.weight"), bb=t("conv_b.bias"))
    got = bref.grads64(x, t("go"), swish)
    keys = dict(f="f", zq="zq", gn_w="norm_layer.weight", gn_b="norm_layer.bias", wy="conv_y.weight", by="conv_y.bias", wb="conv_b.weight", bb="conv_b.bias")
    for k in bref.GRADS:
        want = t(f"grad{int(swish)}/{keys[k]}")
        assert want.dtype == f64 and got[k].shape == want.shape
        assert float((got[k] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k
    # the sub-sampled axis: zq columns 1, 3, 5 are never read and get exactly 0, in the class as in the restatement
    assert bool((t(f"grad{int(swish)}/zq")[..., 1::2] == 0).all()) and bool((got["zq"][..., 1::2] == 0).all())


@pytest.mark.parametrize("swish", [False, True])
def test_with_add_conv_the_gradients_reach_the_3x3_conv_as_in_the_real_class(golden, swish):
    """the module's arrangement for add_conv -- torch's interpolate and 3x3 conv in front, the layer at ratio 1 behind them -- with
    the restatement in the layer's place gives the real class's gradients, the conv's own included"""
    g = golden("spatial_norm_bwd")
    name = "add_conv"
    t = lambda k: torch.from_numpy(g[f"{name}/{k}"]).double()
    f, zq = t("f").requires_grad_(), t("zq").requires_grad_()
    names = [str(k) for k in g[name + "/keys"]]
    p = {k: t(k).requires_grad_() for k in names}
    z = torch.nn.functional.conv2d(torch.nn.functional.interpolate(zq, size=f.shape[-2:], mode="nearest"), p["conv.weight"], p["conv.bias"], padding=1)
    v = bref.layer64(f, z, p["norm_layer.weight"], p["norm_layer.bias"], p["conv_y.weight"], p["conv_y.bias"], p["conv_b.weight"], p["conv_b.bias"],
                     swish=swish)
    got = torch.autograd.grad(v, [f, zq] + [p[k] for k in names], t("go"))
    for k, gk in zip(["f", "zq"] + names, got):
        want = torch.from_numpy(g[f"{name}/grad{int(swish)}/{k}"])
        assert float((gk - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_e_ref_is_positive_and_finite_for_every_gradient(shape):
    """the bar of the GPU tests is never vacuous and never infinite"""
    Cc, Hh, Ww, hq, wq = shape
    for Bb in (1, 4):
        rng = np.random.default_rng(7)
        x = ref.make_inputs(rng, Bb, Cc, Hh, Ww, hq, wq)
        go = bref.make_go(rng, (Bb, Cc, Hh, Ww))
        for swish in (False, True):
            g64, eref = bref.reference(x, go, swish)
            assert all(0 < eref[k] < float("inf") for k in bref.GRADS), eref
            assert all(bool(torch.isfinite(g64[k]).all()) for k in bref.GRADS)
