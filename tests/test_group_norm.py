"""GPU: the plain GroupNorm (+ swish) of csrc/cgic_norm.hip (ABI 21) -- the norm kernels instantiated without zq -- against the
float64 restatement of tests/group_norm_ref.py.

The bar is tests/test_spatial_norm.py's.  ref64 = GroupNorm (+ swish) in float64 on the CPU from the exactly upcast inputs; E_ref =
the max-abs error of torch's own fp32 CPU F.group_norm (+ x * sigmoid(x)) against it.  The kernel's fp32 output must err by at most
BAR (4) * E_ref and its NaN pattern must equal ref64's; a half output must equal .to(half) of the same call's fp32 output bit for
bit.  And on finite inputs group_norm must be torch.equal to spatial_norm with conv_y = 1 (wy = 0, by = 1) and conv_b = 0 on a
finite random zq -- n * 1 + 0 is exact -- with group_norm_train's stats spatial_norm_train's bit for bit: the rounding chain is the
one the modulated kernels' tests already hold.  Every test prints its ratio err / E_ref before it asserts; the measured ones are in
profiles/group_norm.md.
"""
import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import norm
import group_norm_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
TYPES = [(f32, f32), (f16, f32), (f16, f16), (bf16, f32), (bf16, bf16)]

# C, H, W: one channel per group and several, widths that are no multiple of 2, 4 or 8 (every unit, every row tail), a plane of
# more than one apply step; B = 1: two launches, B = 4 (128 groups): one
SHAPES = [(32, 2, 2), (32, 3, 5), (64, 6, 10), (32, 34, 68), (512, 16, 16)]
BIG = (64, 136, 128)                    # a group of 2 x 136 x 128 elements: beyond one workgroup's budget at any batch


def dev(x):
    return {k: v.to(DEV) for k, v in x.items()}


def call(x, **kw):
    return norm.group_norm(x["f"], x["gn_w"], x["gn_b"], **kw)


def modulated(x, zq, train=False, **kw):
    """spatial_norm on the same features with conv_y = 1 and conv_b = 0"""
    C = x["f"].shape[1]
    z, o = torch.zeros(C, 4, device=DEV), torch.zeros(C, device=DEV)
    fn = norm.spatial_norm_train if train else norm.spatial_norm
    return fn(x["f"], zq, x["gn_w"], x["gn_b"], z, o + 1, z, o, **kw)


def check(got, ref64, eref, what):
    err, same_nan = ref.max_err(got, ref64)
    print(f"{what}: err {err:.3e}  E_ref {eref:.3e}  ratio {err / eref if eref else float('nan'):.2f}")
    assert same_nan, what
    assert err <= ref.BAR * eref, (what, err, eref)


_cache = {}


def reference(shape, B, dtype, swish):
    """(inputs on the CPU, a zq at ratio 1, ref64, E_ref) of a shape: computed once, shared, never changed"""
    key = (shape, B, dtype, swish)
    if key not in _cache:
        C, H, W = shape
        base = (shape, B, dtype)
        if base not in _cache:
            rng = np.random.default_rng(3000 + C + 7 * H + W)
            _cache[base] = (ref.make_inputs(rng, B, C, H, W, dtype), ref.make_zq(rng, B, H, W))
        x, zq = _cache[base]
        r64 = ref.restatement(x["f"], x["gn_w"], x["gn_b"], swish=swish)
        _cache[key] = (x, zq, r64, ref.e_ref(r64, x["f"], x["gn_w"], x["gn_b"], swish=swish))
    return _cache[key]


def test_abi_21():
    assert cg._lib.lib().cgic_abi_version() >= 21


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-%dx%d" % s)
def test_every_type_pair_and_swish_against_the_bar_and_the_modulated_kernel(shape, B):
    """B = 1: two launches; B = 4 (128 groups): one -- the form is asked from the library, not from a copied constant"""
    C, H, W = shape
    assert norm.one_launch(f32, B, C, H, W) == (B == 4) and norm.one_launch(f16, B, C, H, W) == (B == 4)
    for dt_in, dt_out in TYPES:
        for swish in (False, True):
            x, zq, r64, eref = reference(shape, B, dt_in, swish)
            xd, zqd = dev(x), zq.to(DEV)
            got32 = call(xd, swish=swish)
            assert got32.dtype == f32 and got32.shape == x["f"].shape
            if dt_out == f32:
                check(got32, r64, eref, f"{shape} B{B} {dt_in} swish={swish}")
                assert torch.equal(got32, modulated(xd, zqd, swish=swish)), (shape, B, dt_in, swish)
                out_t, stats = norm.group_norm_train(xd["f"], xd["gn_w"], xd["gn_b"], swish=swish)
                out_m, stats_m = modulated(xd, zqd, train=True, swish=swish)
                assert torch.equal(out_t, got32) and stats.shape == (B * 32, 2) and stats.dtype == f32
                assert torch.equal(stats.view(torch.int32), stats_m.view(torch.int32))
            else:
                half = call(xd, swish=swish, out_dtype=dt_out)
                assert half.dtype == dt_out and torch.equal(half, got32.to(dt_out))
                assert torch.equal(half, modulated(xd, zqd, swish=swish, out_dtype=dt_out))
                half_t, _ = norm.group_norm_train(xd["f"], xd["gn_w"], xd["gn_b"], swish=swish, out_dtype=dt_out)
                assert torch.equal(half_t, half)


@pytest.mark.parametrize("dtype", [f32, f16])
def test_a_group_beyond_the_budget_takes_two_launches_at_any_batch(dtype):
    C, H, W = BIG
    assert not norm.one_launch(dtype, 1, C, H, W) and not norm.one_launch(dtype, 4, C, H, W) and not norm.one_launch(dtype, 64, C, H, W)
    x, zq, r64, eref = reference(BIG, 1, dtype, True)
    xd = dev(x)
    got = call(xd, swish=True)
    check(got, r64, eref, f"big {dtype}")
    assert torch.equal(got, modulated(xd, zq.to(DEV), swish=True))


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [f32, f16])
def test_views_at_storage_offsets_and_a_given_out(dtype, B):
    """f and out as views 1, 2 and 4 elements into their storage: the narrower units; the same bits as the aligned call, and
    nothing outside the view of out is written"""
    shape = (64, 8, 12)
    x, _, r64, eref = reference(shape, B, dtype, False)
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
            assert bool((ostore[:off] == 7).all()) and bool((ostore[off + n:] == 7).all())
    check(want, r64, eref, f"{shape} B{B} {dtype} views")


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [f32, bf16])
def test_in_place(dtype, B):
    shape = (32, 34, 68) if B == 1 else (64, 6, 10)
    x, _, _, _ = reference(shape, B, dtype, True)
    xd = dev(x)
    want = call(xd, swish=True, out_dtype=dtype)
    f = xd["f"].clone()
    assert call({**xd, "f": f}, swish=True, out=f) is f and torch.equal(f, want)
    if dtype != f32:        # a fp32 result cannot land on half features
        g = xd["f"].clone()
        with pytest.raises(cg.CgicError, match="group_norm: out overlaps an input"):
            cg._lib.call("cgic_group_norm", g.data_ptr(), 2, *x["f"].shape, 32, 1e-6, xd["gn_w"].data_ptr(), xd["gn_b"].data_ptr(), 0, g.data_ptr(), 0,
                         None, 0, None)
        assert torch.equal(g, xd["f"])


def _numerics_inputs(B):
    """[B,64,8,12]: groups of 2 x 96 elements.  Group (0,0): mean 100, std 0.01; (0,1): constant; (0,2): std 1e-3"""
    rng = np.random.default_rng(77)
    x = ref.make_inputs(rng, B, 64, 8, 12)
    f = x["f"].reshape(B, 32, -1)
    g = lambda: torch.from_numpy(rng.standard_normal(f.shape[-1]).astype(np.float32))
    f[0, 0] = 100.0 + 0.01 * g()
    f[0, 1] = 0.37
    f[0, 2] = 1e-3 * g()
    x["f"] = f.reshape(B, 64, 8, 12)
    return x


@pytest.mark.parametrize("B", [1, 4])
def test_hard_statistics(B):
    x = _numerics_inputs(B)
    r64 = ref.restatement(x["f"], x["gn_w"], x["gn_b"])
    check(call(dev(x)), r64, ref.e_ref(r64, x["f"], x["gn_w"], x["gn_b"]), f"hard statistics B{B}")


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
    r64 = ref.restatement(xp["f"], xp["gn_w"], xp["gn_b"])
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
    for shape in ((64, 6, 10), (512, 16, 16)):
        x, _, _, _ = reference(shape, 4, dtype, True)
        xd = dev(x)
        got = call(xd, swish=True)
        assert torch.equal(call(xd, swish=True), got)
        for b in range(4):
            assert torch.equal(call({**xd, "f": xd["f"][b:b + 1]}, swish=True), got[b:b + 1])
        assert torch.equal(call({**xd, "f": xd["f"][1:3]}, swish=True), got[1:3])


@pytest.mark.parametrize("B", [1, 4])
def test_a_captured_graph_replays_on_new_features(B):
    shape = (64, 6, 10)
    x, _, _, _ = reference(shape, B, f32, True)
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
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, call(static, swish=True))


def test_every_plan_refusal_arrives_as_the_python_error_before_a_launch():
    x, _, _, _ = reference((64, 6, 10), 1, f16, False)
    xd = dev(x)
    f, gw, gb = xd["f"], xd["gn_w"], xd["gn_b"]
    before = f.clone()
    with pytest.raises(TypeError, match="group_norm: out_dtype torch.bfloat16"):
        call(xd, out_dtype=bf16)
    with pytest.raises(TypeError, match="group_norm: out is torch.bfloat16"):
        call(xd, out=torch.empty_like(f, dtype=bf16))
    with pytest.raises(ValueError, match="group_norm: 64 channels in 48 groups"):
        call(xd, groups=48)
    with pytest.raises(ValueError, match="group_norm: gn_weight"):
        norm.group_norm(f, gw[:32], gb)
    with pytest.raises(ValueError, match="group_norm: out .* must have f's shape"):
        call(xd, out=torch.empty(1, 64, 6, 12, device=DEV))
    with pytest.raises(TypeError, match="group_norm: features torch.float64"):
        norm.group_norm(f.double(), gw, gb)
    raw = lambda *a: cg._lib.call("cgic_group_norm", *a)
    out, ws = torch.empty_like(f, dtype=f32), torch.empty(4096, dtype=torch.uint8, device=DEV)
    head = (f.data_ptr(), 1, 1, 64, 6, 10, 32, 1e-6, gw.data_ptr(), gb.data_ptr(), 0)
    for text, args in (("group_norm: out_dtype 2 with in_dtype 1", (*head, out.data_ptr(), 2, ws.data_ptr(), 4096, None)),
                       ("group_norm: workspace of 100 bytes, need 768", (*head, out.data_ptr(), 0, ws.data_ptr(), 100, None)),
                       ("group_norm: the workspace is not aligned to 8 bytes", (*head, out.data_ptr(), 0, ws.data_ptr() + 4, 2048, None)),
                       ("group_norm: the workspace overlaps a tensor of the call", (*head, out.data_ptr(), 0, out.data_ptr() + 64, 4096, None)),
                       ("group_norm: a pointer is not aligned to its 2-byte element", (f.data_ptr() + 1, *head[1:], out.data_ptr(), 0, ws.data_ptr(), 4096, None)),
                       ("group_norm: out overlaps an input", (*head, f.data_ptr(), 0, ws.data_ptr(), 4096, None)),
                       ("group_norm: NULL tensor", (*head[:8], None, gb.data_ptr(), 0, out.data_ptr(), 0, ws.data_ptr(), 4096, None)),
                       ("group_norm: eps -1", (*head[:7], -1.0, *head[8:], out.data_ptr(), 0, ws.data_ptr(), 4096, None))):
        with pytest.raises(cg.CgicError, match=text):
            raw(*args)
    with pytest.raises(cg.CgicError, match="group_norm_train: stats overlaps another tensor of the call"):
        cg._lib.call("cgic_group_norm_train", *head, out.data_ptr(), 0, out.data_ptr() + 16, ws.data_ptr(), 4096, None)
    torch.cuda.synchronize()
    assert torch.equal(f, before)


# ---------------------------------------------------------------------------- the module and the ops
def _pair(C=64, seed=5):
    import spatial_norm_ref as sref
    theirs = sref.randomize(torch.nn.GroupNorm(32, C, eps=1e-6), seed).to(DEV)
    return theirs, norm.GroupNorm.adopt(theirs)


@pytest.mark.parametrize("swish", [False, True])
def test_module_under_no_grad_against_the_bar(swish):
    f = torch.from_numpy(np.random.default_rng(21).standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV)
    theirs, mine = _pair()
    with torch.no_grad():
        assert mine.uses_kernel(f) and not mine.uses_backward_kernel(f)
        got = mine(f, swish=swish)
    r64 = ref.restatement(f, theirs.weight, theirs.bias, swish=swish)
    check(got, r64, ref.e_ref(r64, f, theirs.weight, theirs.bias, swish=swish), f"module swish={swish}")
    assert torch.equal(got, norm.group_norm(f, theirs.weight, theirs.bias, swish=swish))


def test_module_with_autograd_takes_the_torch_path_and_an_empty_batch_too():
    f = torch.from_numpy(np.random.default_rng(23).standard_normal((2, 64, 4, 6)).astype(np.float32)).to(DEV).requires_grad_()
    theirs, mine = _pair()
    assert mine._route(f) == "torch"
    got, want = mine(f), theirs(f)
    assert torch.equal(got, want)
    g1, = torch.autograd.grad(got.square().sum(), f, retain_graph=True)
    g2, = torch.autograd.grad(want.square().sum(), f)
    assert torch.equal(g1, g2)
    mine.backward_kernel = True
    assert mine._route(f) == "train" and mine._route(f[:0]) == "torch" and mine(f[:0]).shape == (0, 64, 4, 6)
    with torch.no_grad():
        assert mine._route(f) == "kernel" and mine(f[:0]).shape == (0, 64, 4, 6)


@pytest.mark.parametrize("half", [f16, bf16])
def test_output_dtype_under_autocast_is_torchs(half):
    f = torch.from_numpy(np.random.default_rng(24).standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV).to(half)
    theirs, mine = _pair()
    with torch.no_grad(), torch.autocast("cuda", dtype=half):
        want = theirs(f)
        assert mine.uses_kernel(f)
        got = mine(f)
        opt_in = mine(f, swish=True, out_dtype=half)
        sw32 = mine(f, swish=True)
    assert got.dtype == want.dtype == f32
    assert opt_in.dtype == half and torch.equal(opt_in, sw32.to(half))
    r64 = ref.restatement(f, theirs.weight, theirs.bias)
    check(got, r64, ref.e_ref(r64, f, theirs.weight, theirs.bias), f"module autocast {half}")
    with torch.no_grad():                                       # a half model outside autocast: torch's GroupNorm keeps the type
        hm = norm.GroupNorm.adopt(torch.nn.GroupNorm(32, 64, eps=1e-6).to(DEV).to(half))
        assert hm.uses_kernel(f) and hm(f).dtype == half


@pytest.mark.parametrize("dtype, half_out", [(f32, False), (f16, False), (bf16, True)])
def test_the_ops_agree_with_the_raw_calls(dtype, half_out):
    x, _, _, _ = reference((64, 6, 10), 1, dtype, False)
    xd = dev(x)
    real = torch.ops.cgic.group_norm(xd["f"], xd["gn_w"], xd["gn_b"], 32, 1e-6, True, half_out)
    assert torch.equal(real, call(xd, swish=True, out_dtype=dtype if half_out else None))
    out, stats = torch.ops.cgic.group_norm_train(xd["f"], xd["gn_w"], xd["gn_b"], 32, 1e-6, True, half_out)
    assert torch.equal(out, real) and stats.shape == (32, 2)
