"""GPU: the plain GroupNorm for training (csrc/cgic_norm.hip, csrc/cgic_norm_bwd.hip, ABI 21) -- group_norm_train and group_norm_backward -- against float64
autograd of GroupNorm (+ swish) on the CPU (tests/group_norm_ref.py).

The bar is tests/test_spatial_norm_bwd.py's.  Per gradient tensor (f, gn_weight, gn_bias): g64 = the float64 gradient from the
exactly upcast inputs and a seeded go; E_ref = the max-abs error of torch's fp32 CPU autograd of the same expression against g64.
The kernels' gradient must err by at most BAR (4) * E_ref of that tensor, and its NaN pattern must equal g64's.  A half df must equal
.to(half) of the same call's fp32 df bit for bit.  Every test prints its ratios err / E_ref before it asserts; the measured ones are
in profiles/group_norm.md.
"""
import numpy as np
import pytest
import torch

from control_gic_amd import norm
import group_norm_ref as ref
import spatial_norm_ref as sref
import spatial_norm_bwd_ref as bref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
TYPES = [(f32, f32), (f16, f32), (bf16, f32), (f16, f16), (bf16, bf16)]              # (f, go)
SHAPES = [(32, 2, 2), (32, 3, 5), (64, 6, 10), (32, 34, 68), (512, 16, 16)]
BIG = (64, 136, 128)                    # 17 pixel tiles per plane at unit 4
NAMES = dict(zip(ref.GRADS, norm.GN_GRADS))                                          # the reference's names -> the call's


def dev(x):
    return {k: v.to(DEV) for k, v in x.items()}


_cache = {}


def inputs(shape, B, dtype):
    """(inputs on the CPU, go): drawn once, shared, never changed.  go holds values of `dtype`, as fp32"""
    base = (shape, B, dtype)
    if base not in _cache:
        C, H, W = shape
        rng = np.random.default_rng(4000 + C + 7 * H + W)
        _cache[base] = (ref.make_inputs(rng, B, C, H, W, dtype), bref.make_go(rng, (B, C, H, W), dtype).float())
    return _cache[base]


def reference(shape, B, dtype, swish):
    """(inputs on the CPU, go, {gradient: float64}, {gradient: E_ref}): computed once, shared, never changed"""
    key = (shape, B, dtype, swish)
    if key not in _cache:
        x, go = inputs(shape, B, dtype)
        _cache[key] = (x, go, *ref.reference_grads(x, go, swish))
    return _cache[key]


def train(xd, swish=False, **kw):
    return norm.group_norm_train(xd["f"], xd["gn_w"], xd["gn_b"], swish=swish, **kw)


def backward(xd, go, stats, swish=False, **kw):
    """-> {name in ref.GRADS: gradient or None}"""
    return dict(zip(ref.GRADS, norm.group_norm_backward(go, xd["f"], stats, xd["gn_w"], xd["gn_b"], swish=swish, **kw)))


def check(got, g64, eref, what, names=ref.GRADS):
    """every gradient tensor against its own bar; all the ratios are printed before the first assertion"""
    rows = []
    for k in names:
        err, same_nan = ref.max_err(got[k].reshape(g64[k].shape), g64[k])
        rows.append((k, err, eref[k], same_nan))
    print(what + ": " + "  ".join(f"{k} {err / e if e else float('nan'):.2f}" for k, err, e, _ in rows) + "   (err / E_ref)")
    for k, err, e, same_nan in rows:
        assert same_nan, (what, k)
        assert err <= ref.BAR * e, (what, k, err, e)


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-%dx%d" % s)
def test_every_type_pair_and_swish_against_the_bar(shape, B):
    C, H, W = shape
    assert norm.one_launch(f32, B, C, H, W) == (B == 4)                         # both forms of the training forward
    for dt, dt_go in TYPES:
        for swish in (False, True):
            x, go, g64, eref = reference(shape, B, dt, swish)
            xd, god = dev(x), go.to(DEV).to(dt_go)
            out, stats = train(xd, swish=swish)
            got = backward(xd, god, stats, swish=swish, df_dtype=f32)
            assert all(got[k].dtype == f32 and got[k].shape == xd[k].shape for k in ref.GRADS)
            check(got, g64, eref, f"{shape} B{B} f {dt} go {dt_go} swish={swish}")
            if dt != f32:
                half = backward(xd, god, stats, swish=swish, need=("f",))["f"]
                assert half.dtype == dt and torch.equal(half, got["f"].to(dt))


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("shape, zq_grid, dtype", [((32, 3, 5), (3, 5), f32), ((64, 6, 10), (6, 10), f32), ((32, 34, 68), (17, 17), f32),
                                                   ((512, 16, 16), (16, 16), f16)], ids=["unit1", "unit2", "unit4-zq-up", "unit8-f16"])
def test_the_bits_of_the_modulated_kernels_at_conv_y_1_and_conv_b_0(shape, zq_grid, dtype, B):
    """what csrc/cgic_norm_bwd.hip promises of its two instantiations: on finite inputs group_norm_train + group_norm_backward give
    the bits of spatial_norm_train + spatial_norm_backward with wy = wb = 0, by = 1, bb = 0 on any finite zq (n * 1 + 0 and gv * 1 are
    exact) -- out, stats, df (fp32), dgn_weight and dgn_bias, at every unit, in both forms of the forward, with and without swish.
    go has the features' type"""
    C, H, W = shape
    assert norm.one_launch(dtype, B, C, H, W) == (B == 4)
    x, go = inputs(shape, B, dtype)
    xd, god = dev(x), go.to(DEV).to(dtype)
    zq = ref.make_zq(np.random.default_rng(4100 + C), B, *zq_grid).to(DEV)
    assert bool(torch.isfinite(zq).all())
    conv = (torch.zeros(C, 4, device=DEV), torch.ones(C, device=DEV), torch.zeros(C, 4, device=DEV), torch.zeros(C, device=DEV))    # wy, by, wb, bb
    for swish in (False, True):
        out, stats = train(xd, swish=swish)
        mout, mstats = norm.spatial_norm_train(xd["f"], zq, xd["gn_w"], xd["gn_b"], *conv, swish=swish)
        assert torch.equal(out, mout) and torch.equal(stats, mstats), (shape, B, swish)
        got = backward(xd, god, stats, swish=swish, df_dtype=f32)
        mod = dict(zip(norm.GRADS, norm.spatial_norm_backward(god, xd["f"], zq, mstats, xd["gn_w"], xd["gn_b"], *conv, swish=swish,
                                                              need=("f", "gn_weight", "gn_bias"), df_dtype=f32)))
        for k in ref.GRADS:
            assert got[k].dtype == f32 and torch.equal(got[k], mod[NAMES[k]]), (shape, B, swish, k)
        assert all(mod[k] is None for k in norm.GRADS if k not in norm.GN_GRADS)


@pytest.mark.parametrize("dtype", [f32, f16])
def test_a_span_beyond_one_workgroup(dtype):
    x, go, g64, eref = reference(BIG, 1, dtype, True)
    xd, god = dev(x), go.to(DEV)
    out, stats = train(xd, swish=True)
    assert torch.equal(out, norm.group_norm(xd["f"], xd["gn_w"], xd["gn_b"], swish=True))
    check(backward(xd, god, stats, swish=True, df_dtype=f32), g64, eref, f"big {dtype}")


@pytest.mark.parametrize("dtype", [f32, f16])
def test_two_calls_agree_an_image_alone_gives_its_bits_and_the_workspace_need_not_be_zeroed(dtype):
    for shape in ((64, 6, 10), (32, 34, 68), (512, 16, 16)):
        x, go, _, _ = reference(shape, 4, dtype, True)
        xd, god = dev(x), go.to(DEV)
        _, stats = train(xd, swish=True)
        got = backward(xd, god, stats, swish=True)
        again = backward(xd, god, stats, swish=True)
        assert all(torch.equal(got[k], again[k]) for k in ref.GRADS)
        ws = torch.full((norm.group_norm_backward_workspace_bytes(dtype, 4, *shape) + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        dirty = backward(xd, god, stats, swish=True, workspace=ws)
        assert all(torch.equal(got[k], dirty[k]) for k in ref.GRADS)
        for b in range(4):
            one = {**xd, "f": xd["f"][b:b + 1]}
            _, stats1 = train(one, swish=True)
            assert torch.equal(stats1, stats[32 * b:32 * (b + 1)])
            alone = backward(one, god[b:b + 1], stats1, swish=True, need=("f",))
            assert torch.equal(alone["f"], got["f"][b:b + 1])


@pytest.mark.parametrize("swish", [False, True])
def test_every_subset_of_need_gives_the_full_calls_bits_and_nothing_else(swish):
    x, go, _, _ = reference((64, 6, 10), 4, f16, swish)
    xd, god = dev(x), go.to(DEV)
    _, stats = train(xd, swish=swish)
    full = backward(xd, god, stats, swish=swish)
    for mask in range(1, 8):
        need = tuple(n for i, n in enumerate(norm.GN_GRADS) if mask >> i & 1)
        got = backward(xd, god, stats, swish=swish, need=need)
        for k in ref.GRADS:
            if NAMES[k] in need:
                assert torch.equal(got[k], full[k]), (need, k)
            else:
                assert got[k] is None, (need, k)
    with pytest.raises(ValueError, match="group_norm_backward: need"):
        backward(xd, god, stats, need=())
    with pytest.raises(ValueError, match="group_norm_backward: need"):
        backward(xd, god, stats, need=("f", "zq"))


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [f32, f16])
def test_views_into_padded_storage_canaries_and_df_on_go(dtype, B):
    """f, go and df as views 1, 2 and 4 elements into their storage (the narrower units), the parameter gradients inside canary
    buffers: nothing outside the views changes.  A view offset changes the unit and with it the order of the float64 sums, so these
    gradients are held to the bar, not to the aligned call's bits"""
    shape = (64, 6, 10) if B == 1 else (32, 4, 6)
    x, go, g64, eref = reference(shape, B, dtype, True)
    xd, god = dev(x), go.to(DEV).to(dtype)
    _, stats = train(xd, swish=True)
    want = backward(xd, god, stats, swish=True)
    n = x["f"].numel()

    def padded(src, off, fill, dt):
        store = torch.full((src.numel() + 16,), fill, dtype=dt, device=DEV)
        return store, store[off:off + src.numel()].view(src.shape)

    for off in (1, 2, 4):
        fs, fv = padded(xd["f"], off, 3.0, dtype)
        gs, gv = padded(god, off, 5.0, dtype)
        fv.copy_(xd["f"])
        gv.copy_(god)
        stores = {"f": padded(xd["f"], off, 7.0, dtype), "gn_weight": padded(xd["gn_w"], off, 7.0, f32), "gn_bias": padded(xd["gn_b"], off, 7.0, f32)}
        got = backward({**xd, "f": fv}, gv, stats, swish=True, outs={k: v for k, (_, v) in stores.items()})
        got32 = backward({**xd, "f": fv}, gv, stats, swish=True, df_dtype=f32)
        check({**got, "f": got32["f"]}, g64, eref, f"{shape} B{B} {dtype} views +{off}")
        assert torch.equal(got["f"], got32["f"].to(dtype)) and all(torch.equal(got[k], got32[k]) for k in ref.GRADS[1:])
        for k in ref.GRADS:
            store, view = stores[NAMES[k]]
            assert got[k] is view, (off, k)
            assert bool((store[:off] == 7).all()) and bool((store[off + view.numel():] == 7).all()), (off, k)
        assert bool((fs[:off] == 3).all()) and bool((fs[off + n:] == 3).all()) and torch.equal(fv, xd["f"])
        assert bool((gs[:off] == 5).all()) and bool((gs[off + n:] == 5).all()) and torch.equal(gv, god)
    g2 = god.clone()                    # df on go itself: apply reads a unit of go before it writes that unit of df
    assert backward(xd, g2, stats, swish=True, need=("f",), outs={"f": g2})["f"] is g2 and torch.equal(g2, want["f"])


@pytest.mark.parametrize("swish", [False, True])
def test_a_nan_in_f_reaches_the_gradients_it_reaches_in_the_reference(swish):
    rng = np.random.default_rng(31)
    x = ref.make_inputs(rng, 2, 64, 6, 10)
    go = bref.make_go(rng, (2, 64, 6, 10))
    x["f"][1, 5, 2, 3] = float("nan")
    g64, _ = ref.reference_grads(x, go, swish)
    xd = dev(x)
    _, stats = train(xd, swish=swish)
    got = backward(xd, go.to(DEV), stats, swish=swish)
    for k in ref.GRADS:
        assert torch.equal(torch.isnan(got[k].cpu()).reshape(g64[k].shape), torch.isnan(g64[k])), k
    nan = torch.isnan(got["f"].cpu())
    assert bool(nan[1, 4:6].all()) and int(nan.sum()) == 2 * 60


# ---------------------------------------------------------------------------- the module and the op
def _modules(C=64, seed=5, frozen=False):
    theirs = sref.randomize(torch.nn.GroupNorm(32, C, eps=1e-6), seed)
    if frozen:
        for p in theirs.parameters():
            p.requires_grad_(False)
    mine = norm.GroupNorm.adopt(theirs.to(DEV))
    mine.backward_kernel = True
    return theirs, mine


def _module_reference(m, f, go, swish):
    x = dict(f=f.detach().cpu(), gn_w=m.weight.detach().cpu(), gn_b=m.bias.detach().cpu())
    return ref.reference_grads(x, go.detach().cpu(), swish)


@pytest.mark.parametrize("frozen, swish", [(False, False), (False, True), (True, True)])
def test_module_with_the_flag_under_plain_autograd(frozen, swish):
    rng = np.random.default_rng(41)
    f = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV).requires_grad_()
    go = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV)
    _, mine = _modules(frozen=frozen)
    assert mine.uses_backward_kernel(f) and not mine.uses_kernel(f)
    out = mine(f, swish=swish)
    assert out.grad_fn is not None
    wanted = [(k, p) for k, p in (("gn_w", mine.weight), ("gn_b", mine.bias)) if p.requires_grad]
    assert len(wanted) == (0 if frozen else 2)                                     # frozen parameters: their gradients are skipped
    grads = torch.autograd.grad(out, [f] + [p for _, p in wanted], go)
    got = dict(zip(["f"] + [k for k, _ in wanted], grads))
    g64, eref = _module_reference(mine, f, go, swish)
    check(got, g64, eref, f"module frozen={frozen} swish={swish}", names=list(got))


@pytest.mark.parametrize("half", [f16, bf16])
def test_module_with_the_flag_under_autocast(half):
    """features arrive in the half type, the result and go are fp32, df comes back in the half type: held to the bar of the fp32 CPU
    autograd on the exactly upcast features plus one rounding of df to the half type (test_spatial_norm_bwd.py's rule)"""
    rng = np.random.default_rng(42)
    f = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV).to(half).requires_grad_()
    go = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV)
    _, mine = _modules()
    with torch.autocast("cuda", dtype=half):
        assert mine.uses_backward_kernel(f)
        out = mine(f, swish=True)
    assert out.dtype == f32
    got = dict(zip(ref.GRADS, torch.autograd.grad(out, [f, mine.weight, mine.bias], go)))
    assert got["f"].dtype == half and got["gn_w"].dtype == f32
    g64, eref = _module_reference(mine, f, go, True)
    check(got, g64, eref, f"module autocast {half}", names=ref.GRADS[1:])
    step = 2.0 ** -11 if half == f16 else 2.0 ** -8                                 # half an ulp of the half type, relative
    err = (got["f"].cpu().double() - g64["f"]).abs()
    assert bool((err <= ref.BAR * eref["f"] + step * g64["f"].abs() + 1e-30).all())


def test_a_double_backward_raises():
    f = torch.from_numpy(np.random.default_rng(43).standard_normal((2, 64, 4, 6)).astype(np.float32)).to(DEV).requires_grad_()
    _, mine = _modules()
    out = mine(f)
    with pytest.raises(RuntimeError, match="cgic::group_norm_train is once-differentiable"):
        torch.autograd.grad(out.square().sum(), f, create_graph=True)
    g, = torch.autograd.grad(mine(f).square().sum(), f)                            # the plain backward still works
    assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("B", [1, 4])
def test_a_captured_graph_of_forward_and_backward_replays_on_new_inputs(B):
    shape = (64, 6, 10)
    x, go, _, _ = reference(shape, B, f32, True)
    xd, god = dev(x), go.to(DEV)

    def chain(xs, g, ws):
        out, stats = train(xs, swish=True)
        return out, backward(xs, g, stats, swish=True, workspace=ws)

    ws = torch.empty(norm.group_norm_backward_workspace_bytes(f32, B, *shape), dtype=torch.uint8, device=DEV)
    chain(xd, god, ws)                                          # once eagerly before the capture
    static = {k: v.clone() for k, v in xd.items()}
    sgo = god.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = chain(static, sgo, ws)
    rng = np.random.default_rng(45)
    for _ in range(2):
        static["f"].copy_(torch.from_numpy(rng.standard_normal(x["f"].shape).astype(np.float32)))
        sgo.copy_(torch.from_numpy(rng.standard_normal(x["f"].shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        eager_out, eager = chain(static, sgo, torch.empty_like(ws))
        assert torch.equal(out, eager_out) and all(torch.equal(grads[k], eager[k]) for k in ref.GRADS)
