"""GPU: the fused SpatialNorm (csrc/cgic_norm.hip, ABI 17) against the float64 restatement of the layer (tests/spatial_norm_ref.py,
which tests/test_spatial_norm_host.py holds to the real class's fixture).

The bar.  ref64 = the layer in float64 on the CPU from the exactly upcast inputs; E_ref = the max-abs error of the same expression
by torch's own fp32 CPU ops (F.interpolate, F.group_norm, F.conv2d) against ref64.  The kernel's fp32 output must err by at most
4 * E_ref (both sides are the same chain of about six roundings in another order; a wrong statistic, index or weight is off by 1e-3
or more), and its NaN pattern must equal ref64's.  A half output must equal .to(half) of the same call's fp32 output bit for bit.
Every test prints its ratio err / E_ref before it asserts; the measured ones are in profiles/spatial_norm.md.
"""
import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import norm
import spatial_norm_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
TYPES = [(f32, f32), (f16, f32), (f16, f16), (bf16, f32), (bf16, bf16)]

# name: C, H, W, hq, wq -- the smallest shapes at which each part can go wrong: one channel per group and several, widths that are
# no multiple of 4 or 8 (every unit, every row tail), zq up-sampled x1 x2 x4, sub-sampled 4x and 16x, the axes at different ratios
SHAPES = {
    "C32-2x2-x1": (32, 2, 2, 2, 2),
    "C32-3x5-x1-odd-width": (32, 3, 5, 3, 5),
    "C32-4x6-up2": (32, 4, 6, 2, 3),
    "C64-6x10-down4": (64, 6, 10, 24, 40),
    "C32-8x12-up4": (32, 8, 12, 2, 3),
    "C64-8x12-up2-x1": (64, 8, 12, 4, 12),
    "C64-6x10-down2-up2": (64, 6, 10, 12, 5),
    "C32-34x68-up2-up4": (32, 34, 68, 17, 17),
    "C512-16x16-down16": (512, 16, 16, 64, 64),
}
BIG = (64, 136, 128, 34, 32)            # a group of 2 x 136 x 128 elements: beyond one workgroup's budget at any batch


def dev(x):
    return {k: v.to(DEV) for k, v in x.items()}


def call(x, **kw):
    return norm.spatial_norm(*(x[k] for k in ref.ORDER), **kw)


def check(got, ref64, eref, what):
    err, same_nan = ref.max_err(got, ref64)
    print(f"{what}: err {err:.3e}  E_ref {eref:.3e}  ratio {err / eref if eref else float('nan'):.2f}")
    assert same_nan, what
    assert err <= ref.BAR * eref, (what, err, eref)


_cache = {}


def reference(name, B, dtype, swish):
    """(inputs on the CPU, ref64, E_ref) of a shape: computed once, shared, never changed"""
    key = (name, B, dtype, swish)
    if key not in _cache:
        C, H, W, hq, wq = BIG if name == "big" else SHAPES[name]
        seed = sorted(SHAPES).index(name) if name in SHAPES else 99
        base = (name, B, dtype)
        if base not in _cache:
            _cache[base] = ref.make_inputs(np.random.default_rng(1000 + seed), B, C, H, W, hq, wq, dtype)
        x = _cache[base]
        args = [x[k] for k in ref.ORDER]
        r64 = ref.restatement(*args, swish=swish)
        _cache[key] = (x, r64, ref.e_ref(r64, *args, swish=swish))
    return _cache[key]


def test_abi_17():
    assert cg._lib.lib().cgic_abi_version() >= 17


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_type_pair_and_swish_against_the_bar(name, B):
    """B = 1: two launches; B = 4 (128 groups): one -- the form is asked from the library, not from a copied constant"""
    C, H, W, _, _ = SHAPES[name]
    assert norm.one_launch(f32, B, C, H, W) == (B == 4) and norm.one_launch(f16, B, C, H, W) == (B == 4)
    for dt_in, dt_out in TYPES:
        for swish in (False, True):
            x, r64, eref = reference(name, B, dt_in, swish)
            xd = dev(x)
            got32 = call(xd, swish=swish)
            assert got32.dtype == f32 and got32.shape == x["f"].shape
            if dt_out == f32:
                check(got32, r64, eref, f"{name} B{B} {dt_in} swish={swish}")
            else:
                half = call(xd, swish=swish, out_dtype=dt_out)
                assert half.dtype == dt_out and torch.equal(half, got32.to(dt_out))


@pytest.mark.parametrize("dtype", [f32, f16])
def test_a_group_beyond_the_budget_takes_two_launches_at_any_batch(dtype):
    C, H, W, hq, wq = BIG
    assert not norm.one_launch(dtype, 1, C, H, W) and not norm.one_launch(dtype, 4, C, H, W) and not norm.one_launch(dtype, 64, C, H, W)
    x, r64, eref = reference("big", 1, dtype, True)
    check(call(dev(x), swish=True), r64, eref, f"big {dtype}")


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [f32, f16])
def test_views_at_storage_offsets_and_a_given_out(dtype, B):
    """f and out as views 1, 2 and 4 elements into their storage: the narrower units; the same bits as the aligned call"""
    name = "C64-8x12-up2-x1"
    x, r64, eref = reference(name, B, dtype, False)
    xd = dev(x)
    want = call(xd)
    n = x["f"].numel()
    for off in (1, 2, 4):
        store = torch.zeros(n + 8, dtype=dtype, device=DEV)
        store[off:off + n] = xd["f"].reshape(-1)
        view = store[off:off + n].view(x["f"].shape)
        assert view.storage_offset() == off
        assert torch.equal(call({**xd, "f": view}), want)
        for dt_out in (f32, dtype):
            ostore = torch.full((n + 8,), 7.0, dtype=dt_out, device=DEV)
            out = ostore[off:off + n].view(x["f"].shape)
            assert call(xd, out=out) is out and torch.equal(out, want.to(dt_out))
            assert bool((ostore[:off] == 7).all()) and bool((ostore[off + n:] == 7).all())          # nothing outside the view
    check(want, r64, eref, f"{name} B{B} {dtype} views")


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [f32, bf16])
def test_in_place(dtype, B):
    name = "C32-34x68-up2-up4" if B == 1 else "C64-6x10-down4"
    x, _, _ = reference(name, B, dtype, True)
    xd = dev(x)
    want = call(xd, swish=True, out_dtype=dtype)
    f = xd["f"].clone()
    assert call({**xd, "f": f}, swish=True, out=f) is f and torch.equal(f, want)
    if dtype != f32:        # a fp32 result cannot land on half features
        with pytest.raises(cg.CgicError, match="out overlaps an input"):
            g = xd["f"].clone()
            cg._lib.call("cgic_spatial_norm", g.data_ptr(), 2, *x["f"].shape, xd["zq"].data_ptr(), *x["zq"].shape[2:], 32, 1e-6,
                         *(xd[k].data_ptr() for k in ref.ORDER[2:]), 0, g.data_ptr(), 0, None, 0, None)


def _numerics_inputs(B, dtype=f32):
    """[B,64,8,12]: groups of 2 x 96 elements.  Group (0,0): mean 100, std 0.01; (0,1): constant; (0,2): std 1e-3"""
    rng = np.random.default_rng(77)
    x = ref.make_inputs(rng, B, 64, 8, 12, 4, 6, f32)
    f = x["f"].reshape(B, 32, -1)
    g = lambda: torch.from_numpy(rng.standard_normal(f.shape[-1]).astype(np.float32))
    f[0, 0] = 100.0 + 0.01 * g()
    f[0, 1] = 0.37
    f[0, 2] = 1e-3 * g()
    x["f"] = f.reshape(B, 64, 8, 12).to(dtype)
    return x


@pytest.mark.parametrize("B", [1, 4])
def test_hard_statistics(B):
    """a span far from zero with a small spread, a constant span, a tiny spread: the sums about the span's first element do not cancel"""
    x = _numerics_inputs(B)
    args = [x[k] for k in ref.ORDER]
    r64 = ref.restatement(*args)
    got = call(dev(x))
    check(got, r64, ref.e_ref(r64, *args), f"hard statistics B{B}")
    # span by span as well: each against its own E_ref would be stricter than the issue's bar; the constant span is exact in n
    const = got.reshape(B, 32, -1)[0, 1].cpu().double()
    want = r64.reshape(B, 32, -1)[0, 1]
    assert float((const - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("B", [2, 4])
def test_nan_and_inf_poison_their_span_only(B):
    x = _numerics_inputs(B)
    clean = call(dev(x)).reshape(B, 32, -1)
    f = x["f"].clone().reshape(B, 32, -1)
    f[0, 3, 17] = float("nan")
    f[1, 5, 0] = float("inf")              # (the span's first element: K itself)
    f[1, 7, 100] = float("-inf")
    xp = {**x, "f": f.reshape(x["f"].shape)}
    got = call(dev(xp))
    r64 = ref.restatement(*(xp[k] for k in ref.ORDER))
    assert torch.equal(torch.isnan(got.cpu()), torch.isnan(r64))
    got = got.reshape(B, 32, -1)
    poisoned = torch.zeros(B, 32, dtype=torch.bool)
    poisoned[0, 3] = poisoned[1, 5] = poisoned[1, 7] = True
    assert bool(torch.isnan(got[poisoned.to(DEV)]).all())
    assert torch.equal(got[~poisoned.to(DEV)], clean[~poisoned.to(DEV)])


@pytest.mark.parametrize("dtype", [f32, f16])
def test_two_runs_agree_and_an_image_alone_gives_its_bits_in_the_batch(dtype):
    """the statistics are rounded from float64 sums in a fixed order, so the two forms agree as well: the batch of 4 takes one
    launch, each image alone two"""
    for name in ("C64-8x12-up2-x1", "C512-16x16-down16"):
        x, _, _ = reference(name, 4, dtype, True)
        xd = dev(x)
        got = call(xd, swish=True)
        assert torch.equal(call(xd, swish=True), got)
        for b in range(4):
            alone = call({**xd, "f": xd["f"][b:b + 1], "zq": xd["zq"][b:b + 1]}, swish=True)
            assert torch.equal(alone, got[b:b + 1])
        pair = call({**xd, "f": xd["f"][1:3], "zq": xd["zq"][1:3]}, swish=True)
        assert torch.equal(pair, got[1:3])


# ---------------------------------------------------------------------------- the module, the op, install()
def _module(C, add_conv=False, seed=5):
    m = ref.randomize(ref.StandIn(C, 4, add_conv=add_conv), seed).to(DEV).eval()
    return m, norm.SpatialNorm.adopt(m)


def _module_args(m, f, zq):
    sd = m.state_dict()
    return (f, zq, sd["norm_layer.weight"], sd["norm_layer.bias"], sd["conv_y.weight"], sd["conv_y.bias"], sd["conv_b.weight"], sd["conv_b.bias"])


@pytest.mark.parametrize("swish", [False, True])
def test_module_under_no_grad_against_the_bar(swish):
    rng = np.random.default_rng(21)
    f = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV)
    zq = torch.from_numpy(rng.standard_normal((4, 4, 16, 6)).astype(np.float32)).to(DEV)
    theirs, mine = _module(64)
    with torch.no_grad():
        assert mine.uses_kernel(f, zq)
        got = mine(f, zq, swish=swish)
    args = _module_args(theirs, f, zq)
    r64 = ref.restatement(*args, swish=swish)
    check(got, r64, ref.e_ref(r64, *args, swish=swish), f"module swish={swish}")


def test_module_with_add_conv_runs_the_kernel_at_ratio_one():
    rng = np.random.default_rng(22)
    f = torch.from_numpy(rng.standard_normal((4, 32, 8, 12)).astype(np.float32)).to(DEV)
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)).to(DEV)
    theirs, mine = _module(32, add_conv=True)
    with torch.no_grad():
        assert mine.uses_kernel(f, zq)
        got, want = mine(f, zq), theirs(f, zq)
    # against torch on the device: the 3x3 conv is torch's on both sides; the rest within a few fp32 roundings of values of O(1..10)
    assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def test_module_with_autograd_takes_the_torch_path():
    rng = np.random.default_rng(23)
    f = torch.from_numpy(rng.standard_normal((2, 32, 4, 6)).astype(np.float32)).to(DEV).requires_grad_()
    zq = torch.from_numpy(rng.standard_normal((2, 4, 2, 3)).astype(np.float32)).to(DEV)
    theirs, mine = _module(32)
    assert not mine.uses_kernel(f, zq)
    got, want = mine(f, zq), theirs(f, zq)
    assert torch.equal(got, want)
    g1, = torch.autograd.grad(got.square().sum(), f, retain_graph=True)
    g2, = torch.autograd.grad(want.square().sum(), f)
    assert torch.equal(g1, g2)
    gw = torch.autograd.grad(mine(f, zq, swish=True).sum(), mine.conv_y.weight)[0]
    assert gw.shape == mine.conv_y.weight.shape and bool(torch.isfinite(gw).all())


@pytest.mark.parametrize("half", [f16, bf16])
def test_output_dtype_under_autocast_is_the_torch_expressions(half):
    rng = np.random.default_rng(24)
    f = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV).to(half)      # what a conv under autocast hands on
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)).to(DEV)
    theirs, mine = _module(64)
    with torch.no_grad(), torch.autocast("cuda", dtype=half):
        want = theirs(f, zq)
        assert mine.uses_kernel(f, zq)
        got = mine(f, zq)
        opt_in = mine(f, zq, out_dtype=half)
    assert got.dtype == want.dtype == f32
    assert opt_in.dtype == half and torch.equal(opt_in, got.to(half))
    # the values: autocast rounds conv_y / conv_b to the half type first, the kernel keeps them in fp32 -- within the half type's step
    step = 2.0 ** -10 if half == f16 else 2.0 ** -7
    assert float((got - want).abs().max()) <= 4 * step * float(want.abs().max())


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1, self.norm2 = ref.StandIn(32), ref.StandIn(64, add_conv=True)
        self.plain = torch.nn.GroupNorm(32, 64)


class _Model(torch.nn.Module):
    """what install() touches, as small as it gets, and a decoder of SpatialNorm-shaped modules"""

    def __init__(self):
        super().__init__()
        self.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
        self.encoder = torch.nn.Module()
        self.decoder = torch.nn.Module()
        self.decoder.block = _Block()
        self.decoder.norm_out = ref.StandIn(32)
        self.decoder.avgpool_layer1 = torch.nn.AvgPool2d(4, 4, 0)


def test_install_swaps_the_norms_only_when_asked():
    m = ref.randomize(_Model(), 9).to(DEV).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    cg.install(m)
    d = m.decoder
    assert all(type(n) is ref.StandIn for n in (d.block.norm1, d.block.norm2, d.norm_out))         # the default leaves them alone
    assert isinstance(d.avgpool_layer1, cg.model.AvgPool)
    params = {k: p for k, p in m.named_parameters() if "decoder" in k}
    cg.install(m, patch_norms=True)
    assert all(type(n) is norm.SpatialNorm for n in (d.block.norm1, d.block.norm2, d.norm_out))
    assert type(d.block.plain) is torch.nn.GroupNorm
    after = m.state_dict()
    assert [k for k in after if "decoder" in k] == [k for k in before if "decoder" in k]
    assert all(torch.equal(after[k], before[k]) for k in before if "decoder" in k)
    assert all(p is params[k] for k, p in m.named_parameters() if "decoder" in k)
    cg.install(m, patch_norms=True)                                                              # again: nothing left to swap
    assert type(d.norm_out) is norm.SpatialNorm and type(d.norm_out.norm_layer) is torch.nn.GroupNorm
    rng = np.random.default_rng(25)
    f = torch.from_numpy(rng.standard_normal((4, 32, 8, 12)).astype(np.float32)).to(DEV)
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        got = d.norm_out(f, zq)
    args = _module_args(d.norm_out, f, zq)
    r64 = ref.restatement(*args)
    check(got, r64, ref.e_ref(r64, *args), "installed norm_out")


@pytest.mark.parametrize("B", [1, 4])
def test_a_captured_graph_replays_on_new_features_and_a_new_zq(B):
    name = "C64-8x12-up2-x1"
    x, _, _ = reference(name, B, f32, True)
    xd = dev(x)
    call(xd, swish=True)                                        # once eagerly before the capture
    static = {k: v.clone() for k, v in xd.items()}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static, swish=True)
    rng = np.random.default_rng(26)
    for _ in range(2):
        static["f"].copy_(torch.from_numpy(rng.standard_normal(x["f"].shape).astype(np.float32)))
        static["zq"].copy_(torch.from_numpy(rng.standard_normal(x["zq"].shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, call(static, swish=True))


@pytest.mark.parametrize("dtype, half_out", [(f32, False), (f16, False), (bf16, True)])
def test_the_ops_fake_kernel_agrees_with_the_real_one(dtype, half_out):
    x, _, _ = reference("C32-4x6-up2", 1, dtype, False)
    xd = dev(x)
    args = [xd[k] for k in ref.ORDER]
    real = torch.ops.cgic.spatial_norm(*args, 32, 1e-6, True, half_out)
    assert torch.equal(real, call(xd, swish=True, out_dtype=dtype if half_out else None))
    with FakeTensorMode() as mode:
        fake = torch.ops.cgic.spatial_norm(*(mode.from_tensor(a) for a in args), 32, 1e-6, True, half_out)
    assert fake.shape == real.shape and fake.dtype == real.dtype and fake.device.type == "cuda"
