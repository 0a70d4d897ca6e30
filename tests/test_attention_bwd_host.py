"""CPU: the attention's backward pass (ABI 20) as far as it goes without a device.

  - the shape of the ABI: the three entry points in the header, the library and the ctypes table; the op's schema;
  - the references of the GPU test (tests/attention_bwd_ref.py): the seven formulas in float64 and the precision model agree with
    float64 autograd; the NaN patterns, spelled out by index, hold for float64 autograd and for the model;
  - the feasibility check: on every entry of the GPU catalogue the model alone -- as it stands and under three seeded channel
    permutations, stand-ins for another summation order -- stays within the GPU test's bars, and on every excluded entry it does not;
  - what attention.attention_backward refuses, with the full message, under FakeTensorMode on fake "cuda" tensors;
  - the fake kernel and the autograd registration of torch.ops.cgic.attention_train;
  - AttnBlock.backward_kernel defaults off (adopt() included); with it off the routing is what it was; with it on, which calls reach
    the training path; patch_attention / install set the flag only when asked.
"""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib

attn = sys.modules["control_gic_amd.attention"]          # (the package exports the function attention under the module's name)
import attention_ref as ref
import attention_bwd_ref as bref

f32, f16, bf16, f64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cgic_attention_backward": 22, "cgic_attention_backward_workspace_bytes": 4, "cgic_attention_backward_supported": 5}
B, C, N = 2, 256, 37
CPU_TENSOR = ("control_gic_amd ops run on an MI355X (HIP) device only; got a CPU tensor. "
              "There is deliberately no CPU fallback -- the CPU oracle lives in oracle/ and is test-only.")


# ---------------------------------------------------------------------------- the ABI
def test_abi_20_declares_exports_and_binds_the_three_entry_points():
    assert _lib.lib().cgic_abi_version() >= 20
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgic_hip.h")).read(), flags=re.S)
    assert int(re.search(r"^#define\s+CGIC_ABI_VERSION\s+(\d+)", hdr, re.M).group(1)) >= 20
    for name, nargs in NEW.items():
        args = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr).group(1)
        assert len(args.split(",")) == nargs, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs
        assert hasattr(_lib.lib(), name)
    assert attn.GRADS == ("dq", "dk", "dv") and cg.attention_backward is attn.attention_backward
    assert str(torch.ops.cgic.attention_train.default._schema) == "cgic::attention_train(Tensor q, Tensor k, Tensor v, float scale) -> (Tensor, Tensor)"
    assert str(torch.ops.cgic.attention.default._schema).endswith("bool f32_out) -> Tensor")              # the inference op stays


# ---------------------------------------------------------------------------- the references
@pytest.mark.parametrize("name", ["N6", "N111", "N300-q4", "N300-onehot", "N111-q0"])
def test_the_formulas_and_the_model_agree_with_float64_autograd(name):
    go, q, k, v = bref.make_case(name, 2, 256, f32)
    g64 = bref.grads64(go, q, k, v)
    for got, want in zip(bref.formulas64(go, q, k, v), g64):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for dt, tol in ((f32, 1e-4), (f16, 2e-2), (bf16, 2e-1)):            # (the model in its own precision: no tighter than its roundings)
        go, q, k, v = bref.make_case(name, 2, 256, dt)
        g64 = bref.grads64(go, q, k, v)
        for n, e in bref.errors(bref.grads_model(go, q, k, v), g64).items():
            assert e <= tol * max(1.0, float(g64[bref.GRADS.index(n)].abs().max())), (name, dt, n, e)
    if name == "N111-q0":
        assert not bool(g64[1].any()) and not bool(bref.grads_model(go, q, k, v)[1].any())          # dk is exactly 0
    go, q, k, v = bref.make_case(name, 2, 256, f32)
    for got, want in zip(bref.grads_model(go, q, k, v, scale=0.0), bref.grads64(go, q, k, v, scale=0.0)):
        assert bool(torch.isfinite(got).all()) and float((got - want).abs().max()) <= 1e-5
    assert not bool(bref.grads_model(go, q, k, v, scale=0.0)[0].any()) and not bool(bref.grads_model(go, q, k, v, scale=0.0)[1].any())


@pytest.mark.parametrize("dtype", [f32, bf16])
@pytest.mark.parametrize("which", list(bref.NAN_CASES))
def test_the_nan_patterns_spelled_out_by_index(which, dtype):
    go, q, k, v = bref.nan_case(which, 256, dtype)
    for how, got in (("float64 autograd", bref.grads64(go, q, k, v)), ("the model", bref.grads_model(go, q, k, v))):
        for n, g in zip(bref.GRADS, got):
            want = bref.nan_pattern(bref.NAN_CASES[which][n], 256, 300)
            assert torch.equal(torch.isnan(g), want), (which, how, n, int(torch.isnan(g).sum()), int(want.sum()))


def _model_ratios(name, Cw, Bn, dt, scale=None):
    """the model's error over the bar of the GPU test, per gradient: the worst of the model as it stands and its channel permutations"""
    go, q, k, v = bref.make_case(name, Bn, Cw, dt)
    r = bref.case_refs(go, q, k, v, scale=scale)
    bar = bref.bars(r)
    worst = {n: 0.0 for n in bref.GRADS}
    for perm in [None] + bref.perms(name, Cw):
        e = bref.errors(bref.grads_model(go, q, k, v, scale=scale, perm=perm), r.g64)
        for n in bref.GRADS:
            worst[n] = max(worst[n], e[n] / bar[n] if bar[n] else (0.0 if e[n] == 0 else float("inf")))
    return worst


@pytest.mark.parametrize("batch", bref.BATCHES)
@pytest.mark.parametrize("width", bref.WIDTHS)
@pytest.mark.parametrize("name", [n for n in bref.CASES if n != "N1"])
def test_feasibility(name, width, batch):
    """the bars of the GPU test can be met: the model alone meets them on every entry of the catalogue"""
    for case, Cw, Bn, dt in bref.CATALOGUE:
        if case == name and Cw == width and Bn == batch:
            worst = _model_ratios(name, Cw, Bn, dt)
            print(f"{name} C{Cw} B{Bn} {dt}: " + "  ".join(f"{n} {x:.2f}" for n, x in worst.items()) + "   (model error / bar)")
            assert max(worst.values()) <= 1.0, (name, Cw, Bn, dt, worst)


@pytest.mark.parametrize("scale", [0.0, 0.1, 0.01])
def test_feasibility_of_the_given_scales(scale):
    """... and on the inputs of the GPU test of a given scale"""
    for dt in bref.TYPES:
        worst = _model_ratios("N256", 256, 3, dt, scale)
        print(f"N256 C256 B3 {dt} scale {scale}: " + "  ".join(f"{n} {x:.2f}" for n, x in worst.items()) + "   (model error / bar)")
        assert max(worst.values()) <= 1.0, (dt, scale, worst)


def test_the_excluded_entries_are_infeasible():
    """... and the catalogue is the widest such set: on each excluded entry the model alone misses a bar"""
    assert all(e[0] in bref.CASES and e[1] in bref.WIDTHS and e[2] in bref.BATCHES and e[3] in (f16, bf16) for e in bref.EXCLUDED)
    assert len(bref.CATALOGUE) == len(bref.CASES) * 2 * 2 * 3 - len(bref.EXCLUDED)
    for name, Cw, Bn, dt in sorted(bref.EXCLUDED, key=str):
        assert max(_model_ratios(name, Cw, Bn, dt).values()) > 1.0, (name, Cw, Bn, dt)


def test_n1_the_model_is_within_the_caps():
    for Cw in bref.WIDTHS:
        for dt in bref.TYPES:
            go, q, k, v = bref.make_case("N1", 3, Cw, dt)
            lse = ref.lse64(q, k).float()
            cap_v, cap_q, cap_k = bref.n1_caps(go, q, k, v, lse)
            dq, dk, dv = bref.grads_model(go, q, k, v)
            assert bool(((dv.double() - go.double()).abs() <= cap_v).all())
            assert bool((dq.double().abs() <= cap_q).all()) and bool((dk.double().abs() <= cap_k).all())
            assert float(cap_q.max()) < 1e-2 and float(cap_v.max()) < 1e-5            # (caps that say something: go, q, k, v are N(0,1))


# ---------------------------------------------------------------------------- refusals (FakeTensorMode)
def T(*shape, dtype=f32, device="cuda"):
    return torch.empty(shape, dtype=dtype, device=device)


def bwd(dtype=f32, **over):
    kw = {k: over.pop(k) for k in ("need", "grad_dtype", "outs", "workspace", "scale") if k in over}
    a = dict(go=T(B, C, N, dtype=dtype), q=T(B, C, N, dtype=dtype), k=T(B, C, N, dtype=dtype), v=T(B, C, N, dtype=dtype), out=T(B, C, N, dtype=dtype),
             lse=T(B, N))
    a.update(over)
    return attn.attention_backward(a["go"], a["q"], a["k"], a["v"], a["out"], a["lse"], **kw)


NAME = "attention_backward"
NEED = f"expected names out of {attn.GRADS}, at least one, each once, outs among the needed"
ROWS = [
    ("cpu go", lambda: bwd(go=T(B, C, N, device="cpu")), RuntimeError, CPU_TENSOR),
    ("cpu lse", lambda: bwd(lse=T(B, N, device="cpu")), RuntimeError, CPU_TENSOR),
    ("cpu workspace", lambda: bwd(workspace=T(1 << 20, dtype=torch.uint8, device="cpu")), RuntimeError, CPU_TENSOR),
    ("cpu outs", lambda: bwd(outs={"dq": T(B, C, N, device="cpu")}), RuntimeError, CPU_TENSOR),
    ("fp64 q", lambda: bwd(q=T(B, C, N, dtype=f64)), TypeError, f"{NAME}: q torch.float64 {(B, C, N)}; expected fp32, fp16 or bf16 [B,C,N] or [B,C,H,W]"),
    ("q of two dimensions", lambda: bwd(q=T(C, N)), TypeError, f"{NAME}: q torch.float32 {(C, N)}; expected fp32, fp16 or bf16 [B,C,N] or [B,C,H,W]"),
    ("fp16 go on fp32 inputs", lambda: bwd(go=T(B, C, N, dtype=f16)), ValueError,
     f"{NAME}: go torch.float16 {(B, C, N)} on cuda:0; q is torch.float32 {(B, C, N)} on cuda:0"),
    ("fp32 out of half inputs", lambda: bwd(f16, out=T(B, C, N)), ValueError,
     f"{NAME}: out torch.float32 {(B, C, N)} on cuda:0; q is torch.float16 {(B, C, N)} on cuda:0"),
    ("v of another shape", lambda: bwd(v=T(B, C, N + 1)), ValueError, f"{NAME}: v torch.float32 {(B, C, N + 1)} on cuda:0; q is torch.float32 {(B, C, N)} on cuda:0"),
    ("empty batch", lambda: attn.attention_backward(*(T(0, C, N) for _ in range(5)), T(0, N)), ValueError, f"{NAME}: an empty batch"),
    ("lse of another shape", lambda: bwd(lse=T(B, N + 1)), TypeError,
     f"{NAME}: lse torch.float32 {(B, N + 1)} on cuda:0; expected torch.float32 [{B}, {N}] on cuda:0 (attention(..., lse=True)'s)"),
    ("half lse", lambda: bwd(lse=T(B, N, dtype=f16)), TypeError,
     f"{NAME}: lse torch.float16 {(B, N)} on cuda:0; expected torch.float32 [{B}, {N}] on cuda:0 (attention(..., lse=True)'s)"),
    ("need nothing", lambda: bwd(need=()), ValueError, f"{NAME}: need (), outs (); {NEED}"),
    ("need an unknown name", lambda: bwd(need=("dq", "do")), ValueError, f"{NAME}: need ('dq', 'do'), outs (); {NEED}"),
    ("need a name twice", lambda: bwd(need=("dq", "dq")), ValueError, f"{NAME}: need ('dq', 'dq'), outs (); {NEED}"),
    ("outs that are not needed", lambda: bwd(need=("dq",), outs={"dv": T(B, C, N)}), ValueError, f"{NAME}: need ('dq',), outs ('dv',); {NEED}"),
    ("fp16 gradients of fp32 inputs", lambda: bwd(grad_dtype=f16), TypeError, f"{NAME}: grad_dtype torch.float16; expected the inputs' torch.float32 or torch.float32"),
    ("bf16 gradients of fp16 inputs", lambda: bwd(f16, grad_dtype=bf16), TypeError,
     f"{NAME}: grad_dtype torch.bfloat16; expected the inputs' torch.float16 or torch.float32"),
    ("outs of another shape", lambda: bwd(outs={"dk": T(B, C, N + 1)}), ValueError,
     f"{NAME}: outs['dk'] torch.float32 {(B, C, N + 1)} on cuda:0; expected contiguous torch.float32 {(B, C, N)} on cuda:0"),
    ("outs of two types", lambda: bwd(f16, outs={"dq": T(B, C, N, dtype=f16), "dk": T(B, C, N)}), ValueError,
     f"{NAME}: outs['dk'] torch.float32 {(B, C, N)} on cuda:0; expected contiguous torch.float16 {(B, C, N)} on cuda:0"),
    ("a short workspace", lambda: bwd(workspace=T(100, dtype=torch.uint8)), ValueError,
     f"{NAME}: workspace torch.uint8 of 100 elements; expected contiguous torch.uint8 of at least 304 on cuda:0"),
]


@pytest.mark.parametrize("call, exc, text", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusals_come_before_the_first_data_ptr(call, exc, text):
    with FakeTensorMode():
        with pytest.raises(exc) as got:
            call()
    assert str(got.value) == text


def test_the_workspace_is_delta_alone():
    for dt in (f32, f16, bf16):
        assert attn.backward_workspace_bytes(dt, 2, 512, 4096) == 2 * 4096 * 4
        assert attn.backward_workspace_bytes(dt, 3, 256, 37) == 448 <= 3 * 37 * 64 + 4096
    assert attn.backward_supported(bf16, bf16, 2, 512, 4096) and attn.backward_supported(f16, f32, 1, 256, 1)
    assert not attn.backward_supported(f32, f16, 1, 256, 37) and not attn.backward_supported(f32, f32, 1, 128, 37) and not attn.backward_supported(f64, f64, 1, 256, 37)


def test_the_fake_kernel_and_the_autograd_registration():
    with FakeTensorMode():
        for dt in (f32, f16, bf16):
            out, lse = torch.ops.cgic.attention_train(T(B, C, 5, 7, dtype=dt), T(B, C, 5, 7, dtype=dt), T(B, C, 5, 7, dtype=dt), 0.0625)
            assert tuple(out.shape) == (B, C, 5, 7) and out.dtype == dt and tuple(lse.shape) == (B, 35) and lse.dtype == f32 and lse.device.type == "cuda"
        q = T(B, C, N).requires_grad_()
        out, lse = torch.ops.cgic.attention_train(q, T(B, C, N), T(B, C, N), 0.0625)
        assert out.requires_grad and out.grad_fn is not None and tuple(lse.shape) == (B, N)
        assert not lse.requires_grad and lse.grad_fn is None                          # lse is marked non-differentiable
        with torch.no_grad():
            assert not torch.ops.cgic.attention_train(q, T(B, C, N), T(B, C, N), 0.0625)[0].requires_grad


# ---------------------------------------------------------------------------- the module and install()
def test_the_flag_defaults_off_and_off_is_todays_routing():
    assert attn.AttnBlock.backward_kernel is False
    own, adopted = attn.AttnBlock(C), attn.AttnBlock.adopt(ref.StandIn(C))
    assert own.backward_kernel is False and adopted.backward_kernel is False and "backward_kernel" not in vars(adopted)
    assert inspect.signature(cg.install).parameters["attention_backward"].default is False
    assert inspect.signature(attn.patch_attention).parameters["backward_kernel"].default is False
    with FakeTensorMode():
        q = T(B, C, 5, 7)
        with torch.no_grad():
            assert adopted.uses_kernel(q, q, q) and not adopted.uses_backward_kernel(q, q, q)
        g = T(B, C, 5, 7).requires_grad_()
        assert not adopted.uses_kernel(g, q, q) and not adopted.uses_backward_kernel(g, q, q) and adopted._route(g, q, q) == "torch"
    # on the CPU, with autograd, the module is the reference's expression bit for bit, flag or no flag
    theirs = ref.randomize(ref.StandIn(64), 3)
    mine = attn.AttnBlock.adopt(theirs)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 64, 4, 6)).astype(np.float32)).requires_grad_()
    for flag in (False, True):
        mine.backward_kernel = flag
        got, want = mine(x), theirs(x)
        assert torch.equal(got, want) and torch.equal(torch.autograd.grad(got.sum(), x)[0], torch.autograd.grad(want.sum(), x)[0])


def test_with_the_flag_on_the_calls_that_need_a_gradient_reach_the_training_path():
    m = attn.AttnBlock.adopt(ref.StandIn(C))
    m.backward_kernel = True
    with FakeTensorMode():
        q, g = T(B, C, 5, 7), T(B, C, 5, 7).requires_grad_()
        assert m.uses_backward_kernel(g, q, q) and m.uses_backward_kernel(q, q, g) and not m.uses_kernel(g, q, q)
        for dt in (f16, bf16):
            assert m.uses_backward_kernel(T(B, C, 5, 7, dtype=dt).requires_grad_(), T(B, C, 5, 7, dtype=dt), T(B, C, 5, 7, dtype=dt))
        assert m.uses_kernel(q, q, q) and not m.uses_backward_kernel(q, q, q)             # nothing needs a gradient: the inference kernel
        with torch.no_grad():
            assert m.uses_kernel(g, q, q) and not m.uses_backward_kernel(g, q, q)
        # what the kernels do not serve stays on torch's path
        assert m._route(T(B, 128, 5, 7).requires_grad_(), T(B, 128, 5, 7), T(B, 128, 5, 7)) == "torch"          # a width that is not built
        assert m._route(T(0, C, 5, 7).requires_grad_(), T(0, C, 5, 7), T(0, C, 5, 7)) == "torch"                # an empty batch
        assert m._route(T(B, C, 5, 7, dtype=f64).requires_grad_(), T(B, C, 5, 7, dtype=f64), T(B, C, 5, 7, dtype=f64)) == "torch"
        assert m._route(T(B, C, 5, 7, device="cpu").requires_grad_(), T(B, C, 5, 7, device="cpu"), T(B, C, 5, 7, device="cpu")) == "torch"
        assert m._route(g, T(B, C, 5, 7, dtype=f16), q) == "torch"


def test_patch_attention_and_install_set_the_flag_only_when_asked():
    holder = torch.nn.Module()
    holder.a, holder.b = ref.StandIn(32), torch.nn.Sequential(ref.StandIn(64), torch.nn.GroupNorm(32, 64))
    assert attn.patch_attention(holder) == 2 and holder.a.backward_kernel is False and holder.b[0].backward_kernel is False
    assert attn.patch_attention(holder, backward_kernel=True) == 0              # nothing left to swap; the flag reaches those swapped before
    assert holder.a.backward_kernel is True and holder.b[0].backward_kernel is True
    assert attn.AttnBlock.backward_kernel is False                              # the class is untouched
    with pytest.raises(ValueError, match="attention_backward=True sets AttnBlock.backward_kernel on the blocks that patch_attention=True swaps in"):
        model = torch.nn.Module()
        model.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
        model.encoder = torch.nn.Module()
        cg.install(model, attention_backward=True)
