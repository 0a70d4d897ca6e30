"""GPU: SpatialNorm for training (csrc/cgic_norm.hip, csrc/cgic_norm_bwd.hip, ABI 19) -- the forward that keeps the statistics and the backward -- against
float64 autograd of the layer on the CPU (tests/spatial_norm_bwd_ref.py, which tests/test_spatial_norm_bwd_host.py holds to the real
class's gradients).

The bar.  Per gradient tensor (f, zq and the six parameters): g64 = the float64 gradient from the exactly upcast inputs and a
seeded go; E_ref = the max-abs error of torch's fp32 CPU autograd of the same expression against g64.  The kernels' gradient must err
by at most spatial_norm_ref.BAR (4) * E_ref of that tensor, and its NaN pattern must equal g64's.  A half df must equal .to(half) of
the same call's fp32 df bit for bit.  Every test prints its ratios err / E_ref before it asserts; the measured ones are in
profiles/spatial_norm_backward.md.  +-Inf in f or go is not specified (torch's own GroupNorm backward uses another algebra there).
"""
import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import norm
import spatial_norm_ref as ref
import spatial_norm_bwd_ref as bref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
TYPES = [(f32, f32), (f16, f32), (bf16, f32), (f16, f16), (bf16, bf16)]              # (f, go)

# name: C, H, W, hq, wq -- one and several channels per group, odd widths, every unit, up x2 / x4, down x4 / x16, mixed axes; at
# B = 1 the training forward takes two launches, at B = 4 (128 groups) one
SHAPES = {
    "C32-2x2-x1": (32, 2, 2, 2, 2),
    "C32-3x5-x1-odd-width": (32, 3, 5, 3, 5),
    "C32-4x6-up2": (32, 4, 6, 2, 3),
    "C64-6x10-down4": (64, 6, 10, 24, 40),
    "C64-6x10-down2-up2": (64, 6, 10, 12, 5),
    "C32-34x68-up2-up4": (32, 34, 68, 17, 17),
    "C512-16x16-down4": (512, 16, 16, 64, 64),
}
BIG = (64, 136, 128, 34, 32)            # a group of 2 x 136 x 128 elements: beyond one workgroup, 17 pixel tiles per plane


def dev(x):
    return {k: v.to(DEV) for k, v in x.items()}


_cache = {}


def reference(name, B, dtype, swish):
    """(inputs on the CPU, go, {gradient: float64}, {gradient: E_ref}) of a shape: computed once, shared, never changed.  go holds
    values of `dtype`, as fp32"""
    key = (name, B, dtype, swish)
    if key not in _cache:
        C, H, W, hq, wq = BIG if name == "big" else SHAPES[name]
        seed = sorted(SHAPES).index(name) if name in SHAPES else 99
        base = (name, B, dtype)
        if base not in _cache:
            rng = np.random.default_rng(2000 + seed)
            _cache[base] = (ref.make_inputs(rng, B, C, H, W, hq, wq, dtype), bref.make_go(rng, (B, C, H, W), dtype).float())
        x, go = _cache[base]
        _cache[key] = (x, go, *bref.reference(x, go, swish))
    return _cache[key]


def train(xd, swish=False, **kw):
    return norm.spatial_norm_train(*(xd[k] for k in ref.ORDER), swish=swish, **kw)


def backward(xd, go, stats, swish=False, **kw):
    """-> {name in bref.GRADS: gradient or None}"""
    got = norm.spatial_norm_backward(go, xd["f"], xd["zq"], stats, *(xd[k] for k in ref.ORDER[2:]), swish=swish, **kw)
    return dict(zip(bref.GRADS, got))


def check(got, g64, eref, what, names=bref.GRADS):
    """every gradient tensor against its own bar; all the ratios are printed before the first assertion"""
    rows = []
    for k in names:
        err, same_nan = ref.max_err(got[k].reshape(g64[k].shape), g64[k])
        rows.append((k, err, eref[k], same_nan))
    print(what + ": " + "  ".join(f"{k} {err / e if e else float('nan'):.2f}" for k, err, e, _ in rows) + "   (err / E_ref)")
    for k, err, e, same_nan in rows:
        assert same_nan, (what, k)
        assert err <= ref.BAR * e, (what, k, err, e)


def test_abi_19():
    assert cg._lib.lib().cgic_abi_version() >= 19


def ulps(a, b):
    """distance in representable fp32 values"""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_type_pair_and_swish_against_the_bar(name, B):
    C, H, W, _, _ = SHAPES[name]
    assert norm.one_launch(f32, B, C, H, W) == (B == 4)                         # both forms of the training forward
    for dt, dt_go in TYPES:
        for swish in (False, True):
            x, go, g64, eref = reference(name, B, dt, swish)
            xd, god = dev(x), go.to(DEV).to(dt_go)
            out, stats = train(xd, swish=swish)
            if dt_go == f32:                                                    # the training forward, once per feature type
                assert torch.equal(out, norm.spatial_norm(*(xd[k] for k in ref.ORDER), swish=swish))
                if dt != f32:
                    half, stats_h = train(xd, swish=swish, out_dtype=dt)
                    assert torch.equal(half, out.to(dt)) and torch.equal(stats_h, stats)
                f64 = x["f"].double().reshape(B, 32, -1)
                mean = f64.mean(dim=-1)
                rstd = 1.0 / torch.sqrt(((f64 - mean[..., None]) ** 2).mean(dim=-1) + 1e-6)
                want = torch.stack([mean.reshape(-1), rstd.reshape(-1)], dim=1).float()
                assert stats.shape == (B * 32, 2) and stats.dtype == f32 and ulps(stats.cpu(), want) <= 1
            got = backward(xd, god, stats, swish=swish, df_dtype=f32)
            assert got["f"].dtype == f32 and all(got[k].dtype == f32 and got[k].shape == xd[k].shape for k in bref.GRADS)
            check(got, g64, eref, f"{name} B{B} f {dt} go {dt_go} swish={swish}")
            if dt != f32:
                half = backward(xd, god, stats, swish=swish, need=("f",))["f"]
                assert half.dtype == dt and torch.equal(half, got["f"].to(dt))


@pytest.mark.parametrize("dtype", [f32, f16])
def test_a_span_beyond_one_workgroup(dtype):
    x, go, g64, eref = reference("big", 1, dtype, True)
    xd, god = dev(x), go.to(DEV)
    out, stats = train(xd, swish=True)
    assert torch.equal(out, norm.spatial_norm(*(xd[k] for k in ref.ORDER), swish=True))
    check(backward(xd, god, stats, swish=True, df_dtype=f32), g64, eref, f"big {dtype}")


@pytest.mark.parametrize("dtype", [f32, f16])
def test_two_calls_agree_an_image_alone_gives_its_bits_and_the_workspace_need_not_be_zeroed(dtype):
    for name in ("C64-6x10-down2-up2", "C32-34x68-up2-up4", "C512-16x16-down4"):
        x, go, _, _ = reference(name, 4, dtype, True)
        xd, god = dev(x), go.to(DEV)
        _, stats = train(xd, swish=True)
        got = backward(xd, god, stats, swish=True)
        again = backward(xd, god, stats, swish=True)
        assert all(torch.equal(got[k], again[k]) for k in bref.GRADS)
        C, H, W, _, _ = SHAPES[name]
        ws = torch.full((norm.backward_workspace_bytes(dtype, 4, C, H, W) + 64,), 0xFF, dtype=torch.uint8, device=DEV)
        dirty = backward(xd, god, stats, swish=True, workspace=ws)
        assert all(torch.equal(got[k], dirty[k]) for k in bref.GRADS)
        for b in range(4):
            one = {**xd, "f": xd["f"][b:b + 1], "zq": xd["zq"][b:b + 1]}
            _, stats1 = train(one, swish=True)
            assert torch.equal(stats1, stats[32 * b:32 * (b + 1)])
            alone = backward(one, god[b:b + 1], stats1, swish=True, need=("f", "zq"))
            assert torch.equal(alone["f"], got["f"][b:b + 1]) and torch.equal(alone["zq"], got["zq"][b:b + 1])


@pytest.mark.parametrize("swish", [False, True])
def test_outputs_that_are_not_wanted_are_not_computed(swish):
    name = "C64-6x10-down2-up2"
    x, go, _, _ = reference(name, 4, f16, swish)
    xd, god = dev(x), go.to(DEV)
    _, stats = train(xd, swish=swish)
    full = backward(xd, god, stats, swish=swish)
    only_df = backward(xd, god, stats, swish=swish, need=("f",))
    assert torch.equal(only_df["f"], full["f"]) and all(only_df[k] is None for k in bref.GRADS[1:])
    rest = backward(xd, god, stats, swish=swish, need=norm.GRADS[1:])
    assert rest["f"] is None and all(torch.equal(rest[k], full[k]) for k in bref.GRADS[1:])
    frozen = backward(xd, god, stats, swish=swish, need=("f", "wy", "by", "wb", "bb"))            # a frozen GroupNorm, zq without gradient
    assert frozen["zq"] is None and frozen["gn_w"] is None and all(torch.equal(frozen[k], full[k]) for k in ("f", "wy", "by", "wb", "bb"))


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("dtype", [f32, f16])
def test_views_into_padded_storage_and_canaries_around_every_output(dtype, B):
    """f, go and df as views 1, 2 and 4 elements into their storage (the narrower units); dzq and the parameter gradients inside
    canary buffers: nothing outside the views changes.  A view offset changes the unit and with it the order of the float64 sums (the
    plan fixes it per unit), so these gradients are held to the bar, not to the aligned call's bits; the half df to .to(half) of the
    fp32 df of a second call at the same offsets, which also repeats every other gradient bit for bit"""
    name = "C64-6x10-down2-up2" if B == 1 else "C32-4x6-up2"
    C, H, W, hq, wq = SHAPES[name]
    x, go, g64, eref = reference(name, B, dtype, True)
    xd, god = dev(x), go.to(DEV).to(dtype)
    _, stats = train(xd, swish=True)
    want = backward(xd, god, stats, swish=True)
    n = x["f"].numel()

    def padded(src, off, fill, dt):
        store = torch.full((src.numel() + 16,), fill, dtype=dt, device=DEV)
        view = store[off:off + src.numel()].view(src.shape)
        return store, view

    for off in (1, 2, 4):
        fs, fv = padded(xd["f"], off, 3.0, dtype)
        gs, gv = padded(god, off, 5.0, dtype)
        fv.copy_(xd["f"])
        gv.copy_(god)
        stores = {"f": padded(xd["f"], off, 7.0, dtype)}
        for k, nk in zip(bref.GRADS[1:], norm.GRADS[1:]):
            stores[nk] = padded(xd[k], off, 7.0, f32)
        outs = {nk: v for nk, (_, v) in stores.items()}
        got = backward({**xd, "f": fv}, gv, stats, swish=True, outs=outs)
        got32 = backward({**xd, "f": fv}, gv, stats, swish=True, df_dtype=f32)
        check({**got, "f": got32["f"]}, g64, eref, f"{name} B{B} {dtype} views +{off}")
        assert torch.equal(got["f"], got32["f"].to(dtype)) and all(torch.equal(got[k], got32[k]) for k in bref.GRADS[1:])
        for k, nk in zip(bref.GRADS, norm.GRADS):
            store, view = stores[nk]
            assert got[k] is view, (off, k)
            m = view.numel()
            assert bool((store[:off] == 7).all()) and bool((store[off + m:] == 7).all()), (off, k)
        assert bool((fs[:off] == 3).all()) and bool((fs[off + n:] == 3).all()) and torch.equal(fv, xd["f"])
        assert bool((gs[:off] == 5).all()) and bool((gs[off + n:] == 5).all()) and torch.equal(gv, god)
    # df on go itself (equal types, the aligned call's unit): apply reads a unit of go before it writes that unit of df
    g2 = god.clone()
    assert backward(xd, g2, stats, swish=True, need=("f",), outs={"f": g2})["f"] is g2 and torch.equal(g2, want["f"])


def test_zq_elements_that_a_sub_sampled_axis_never_reads_get_exactly_zero():
    for name in ("C64-6x10-down4", "C64-6x10-down2-up2", "C512-16x16-down4"):
        C, H, W, hq, wq = SHAPES[name]
        x, go, g64, _ = reference(name, 4, f32, True)
        xd = dev(x)
        _, stats = train(xd, swish=True)
        dzq = backward(xd, go.to(DEV), stats, swish=True, need=("zq",))["zq"].cpu()
        read = torch.zeros(hq, wq, dtype=torch.bool)
        read[ref.nearest(H, hq)[:, None], ref.nearest(W, wq)[None, :]] = True
        assert bool((dzq[:, :, ~read] == 0).all()) and bool((g64["zq"][:, :, ~read] == 0).all())
        assert bool((dzq[:, :, read] != 0).all()) and int((~read).sum()) > 0


@pytest.mark.parametrize("swish", [False, True])
def test_a_nan_in_f_reaches_the_gradients_it_reaches_in_the_reference(swish):
    C, H, W, hq, wq = SHAPES["C64-6x10-down2-up2"]
    rng = np.random.default_rng(31)
    x = ref.make_inputs(rng, 2, C, H, W, hq, wq)
    go = bref.make_go(rng, (2, C, H, W))
    x["f"][1, 5, 2, 3] = float("nan")
    g64, _ = bref.reference(x, go, swish)
    xd = dev(x)
    _, stats = train(xd, swish=swish)
    got = backward(xd, go.to(DEV), stats, swish=swish)
    for k in bref.GRADS:
        nan = torch.isnan(got[k].cpu()).reshape(g64[k].shape)
        assert torch.equal(nan, torch.isnan(g64[k])), k
    # by index: group 2 of image 1 (channels 4 and 5) and nothing else of df; every zq element of image 1 that is read
    nan = torch.isnan(got["f"].cpu())
    assert bool(nan[1, 4:6].all()) and int(nan.sum()) == 2 * H * W
    assert bool(torch.isnan(got["gn_w"].cpu())[4:6].all()) and int(torch.isnan(got["gn_w"]).sum()) == 2
    assert int(torch.isnan(got["gn_b"]).sum()) == (2 if swish else 0) and int(torch.isnan(got["bb"]).sum()) == (2 if swish else 0)
    assert not bool(torch.isnan(got["zq"][0]).any()) and bool(torch.isnan(got["zq"][1, :, ::2, :]).all())


# ---------------------------------------------------------------------------- the module, the op, install()
def _modules(C, add_conv=False, seed=5, frozen=False):
    theirs = ref.randomize(ref.StandIn(C, 4, add_conv=add_conv), seed)
    if frozen:
        for p in theirs.norm_layer.parameters():
            p.requires_grad_(False)
    mine = norm.SpatialNorm.adopt(theirs.to(DEV))
    mine.backward_kernel = True
    return theirs, mine


def _module_reference(m, f, zq, go, swish):
    """float64 autograd of the module's own expression on the CPU (its 3x3 conv included), and the fp32 CPU one: ({name: g64}, {name: E_ref})"""
    res = []
    for dt in (torch.float64, torch.float32):
        mm = ref.StandIn(m.conv_y.out_channels, 4, add_conv=m.add_conv).to(dt)
        mm.load_state_dict({k: v.detach().cpu().to(dt) for k, v in m.state_dict().items()})
        ff, zz = f.detach().cpu().to(dt).requires_grad_(), zq.detach().cpu().to(dt).requires_grad_()
        v = mm(ff, zz)
        if swish:
            v = v * torch.sigmoid(v)
        names = ["f", "zq"] + [k for k, _ in mm.named_parameters()]
        res.append(dict(zip(names, torch.autograd.grad(v, [ff, zz] + list(mm.parameters()), go.detach().cpu().to(dt)))))
    g64, g32 = res
    return g64, {k: float((g32[k].double() - g64[k]).abs().max()) for k in g64}


@pytest.mark.parametrize("add_conv, frozen, swish", [(False, False, False), (False, False, True), (True, False, True), (False, True, False)])
def test_module_with_the_flag_under_plain_autograd(add_conv, frozen, swish):
    rng = np.random.default_rng(41)
    f = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV).requires_grad_()
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)).to(DEV).requires_grad_()
    go = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV)
    theirs, mine = _modules(64, add_conv=add_conv, frozen=frozen)
    assert mine.uses_backward_kernel(f, zq) and not mine.uses_kernel(f, zq)
    out = mine(f, zq, swish=swish)
    assert out.grad_fn is not None
    wanted = [(k, p) for k, p in mine.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(out, [f, zq] + [p for _, p in wanted], go)
    got = dict(zip(["f", "zq"] + [k for k, _ in wanted], grads))
    g64, eref = _module_reference(mine, f, zq, go, swish)
    assert set(got) == set(g64) - ({"norm_layer.weight", "norm_layer.bias"} if frozen else set())
    check(got, g64, eref, f"module add_conv={add_conv} frozen={frozen} swish={swish}", names=list(got))


@pytest.mark.parametrize("half", [f16, bf16])
def test_module_with_the_flag_under_autocast(half):
    """features arrive in the half type (a conv's output under autocast), the result and go are fp32, df comes back in the half type:
    held to the bar of the fp32 CPU autograd on the exactly upcast features plus one rounding of df to the half type"""
    rng = np.random.default_rng(42)
    f = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV).to(half).requires_grad_()
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)).to(DEV).requires_grad_()
    go = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32)).to(DEV)
    theirs, mine = _modules(64)
    with torch.autocast("cuda", dtype=half):
        assert mine.uses_backward_kernel(f, zq)
        out = mine(f, zq, swish=True)
    assert out.dtype == f32
    names = ["f", "zq"] + [k for k, _ in mine.named_parameters()]
    got = dict(zip(names, torch.autograd.grad(out, [f, zq] + list(mine.parameters()), go)))
    assert got["f"].dtype == half and got["zq"].dtype == f32
    g64, eref = _module_reference(mine, f, zq, go, True)
    check(got, g64, eref, f"module autocast {half}", names=names[1:])
    step = 2.0 ** -11 if half == f16 else 2.0 ** -8                                 # half an ulp of the half type, relative
    err = (got["f"].cpu().double() - g64["f"]).abs()
    assert bool((err <= ref.BAR * eref["f"] + step * g64["f"].abs() + 1e-30).all())


def test_a_double_backward_raises():
    rng = np.random.default_rng(43)
    f = torch.from_numpy(rng.standard_normal((2, 32, 4, 6)).astype(np.float32)).to(DEV).requires_grad_()
    zq = torch.from_numpy(rng.standard_normal((2, 4, 2, 3)).astype(np.float32)).to(DEV)
    _, mine = _modules(32)
    out = mine(f, zq)
    with pytest.raises(RuntimeError, match="once-differentiable"):
        torch.autograd.grad(out.square().sum(), f, create_graph=True)
    g, = torch.autograd.grad(mine(f, zq).square().sum(), f)                        # the plain backward still works
    assert bool(torch.isfinite(g).all())


class _Block(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1, self.norm2 = ref.StandIn(32), ref.StandIn(64, add_conv=True)
        self.conv = torch.nn.Conv2d(32, 64, 3, padding=1)


class _Model(torch.nn.Module):
    """what install() touches, as small as it gets, and a decoder of two SpatialNorm-shaped modules around a conv"""

    def __init__(self):
        super().__init__()
        self.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
        self.encoder = torch.nn.Module()
        self.decoder = torch.nn.Module()
        self.decoder.block = _Block()

    def decode(self, f, zq):
        b = self.decoder.block
        h = b.norm1(f, zq)
        h = b.conv(h * torch.sigmoid(h))
        return b.norm2(h, zq)


def test_install_with_norm_backward_trains_one_sgd_step_as_the_torch_path_does():
    """the same model twice: norms on torch's path, norms on the kernels; one SGD step each from the same state.  The bar: a parameter
    moves by lr * gradient, and the two fp32 gradients are each within BAR * E_ref of the float64 one, E_ref measured here as the
    difference of torch's fp32 gradient on the device to float64 autograd on the CPU"""
    import copy
    rng = np.random.default_rng(44)
    f = torch.from_numpy(rng.standard_normal((4, 32, 8, 12)).astype(np.float32))
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32))
    base = ref.randomize(_Model(), 9)
    lr = 0.05
    ends, grads = {}, {}
    for how in ("cpu64", "torch", "kernel"):
        m = copy.deepcopy(base)
        m = m.double() if how == "cpu64" else m.to(DEV)
        if how != "cpu64":
            cg.install(m, patch_norms=True, norm_backward=(how == "kernel"))
            d = m.decoder.block
            assert type(d.norm1) is norm.SpatialNorm and d.norm1.backward_kernel == (how == "kernel") and d.norm2.backward_kernel == (how == "kernel")
        params = [p for k, p in m.named_parameters() if k.startswith("decoder")]
        opt = torch.optim.SGD(params, lr=lr)
        ff, zz = (f.double(), zq.double()) if how == "cpu64" else (f.to(DEV), zq.to(DEV))
        loss = _Model.decode(m, ff, zz).square().mean()
        opt.zero_grad()
        loss.backward()
        grads[how] = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if k.startswith("decoder")}
        opt.step()
        ends[how] = {k: p.detach().cpu().double() for k, p in m.named_parameters() if k.startswith("decoder")}
    rows = []
    for what, got in (("end", ends), ("grad", grads)):          # the parameters after the step, and the gradients that moved them
        for k, want in got["cpu64"].items():
            e = float((got["torch"][k] - want).abs().max())
            err = float((got["kernel"][k] - want).abs().max())
            rows.append((what + " " + k[len("decoder.block."):], err, e))
    print("  ".join(f"{k} {err / e if e else float('nan'):.2f}" for k, err, e in rows) + "   (err / E_ref)")
    for k, err, e in rows:
        assert 0 < e and err <= ref.BAR * e, (k, err, e)
    assert all(not torch.equal(ends["kernel"][k], base.state_dict()[k].double()) for k in ends["kernel"])          # every parameter moved


@pytest.mark.parametrize("B", [1, 4])
def test_a_captured_graph_of_forward_and_backward_replays_on_new_inputs(B):
    name = "C64-6x10-down2-up2"
    x, go, _, _ = reference(name, B, f32, True)
    xd, god = dev(x), go.to(DEV)

    def chain(xs, g, ws):
        out, stats = train(xs, swish=True)
        return out, backward(xs, g, stats, swish=True, workspace=ws)

    C, H, W, _, _ = SHAPES[name]
    ws = torch.empty(norm.backward_workspace_bytes(f32, B, C, H, W), dtype=torch.uint8, device=DEV)
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
        static["zq"].copy_(torch.from_numpy(rng.standard_normal(x["zq"].shape).astype(np.float32)))
        sgo.copy_(torch.from_numpy(rng.standard_normal(x["f"].shape).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        eager_out, eager = chain(static, sgo, torch.empty_like(ws))
        assert torch.equal(out, eager_out) and all(torch.equal(grads[k], eager[k]) for k in bref.GRADS)
