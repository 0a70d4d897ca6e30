"""GPU: cg.ResnetBlock (control_gic_amd/resblock.py) on the library's norm kernels with the swish fused -- against the fixture of
the REAL ResnetBlocks (tests/golden/resblock.npz; tests/test_resblock_host.py holds the CPU side to it) and against float64 on the CPU.

The bars.  A fixture case on the device must err by at most BAR (4) times the fixture's own fp32 error against its float64 output.
Where there is no fixture (training, the small encoder), E_ref is measured in the test: the error of the same modules on torch's
route on the device against float64 on the CPU; the kernel route must err by at most BAR * E_ref, tensor by tensor.  Every test
prints its ratios before it asserts.
"""
import copy

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import norm
import group_norm_ref as gref
import spatial_norm_ref as sref
from test_resblock_host import CASES, build, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
BAR = gref.BAR


@pytest.mark.parametrize("name", CASES)
def test_every_fixture_case_on_the_device(name):
    kw, sd, x, zq, ref64, err32, keys = load(name)
    m, _, _ = build(name)
    m = m.to(DEV)
    xd, zqd = x.to(DEV), None if zq is None else zq.to(DEV)
    with torch.no_grad():
        assert m.uses_kernel(xd, zqd)                               # library norms: both on the kernel, swish fused
        got = m(xd, None) if zq is None else m(xd, None, zqd)
    err = float((got.cpu().double() - ref64).abs().max())
    print(f"{name}: err {err:.3e}  fixture fp32 {err32:.3e}  ratio {err / err32:.2f}")
    assert got.dtype == f32 and err <= BAR * err32


def _hook_inputs(block):
    """the tensors that enter conv1 and conv2, as the block hands them over (before autocast's own cast inside the conv), and what
    conv1 returns"""
    seen = {}
    hooks = [conv.register_forward_pre_hook(lambda mod, args, k=k: seen.__setitem__(k, args[0])) for k, conv in (("conv1", block.conv1), ("conv2", block.conv2))]
    hooks.append(block.conv1.register_forward_hook(lambda mod, args, out: seen.__setitem__("conv1_out", out)))
    return seen, hooks


@pytest.mark.parametrize("half", [f16, bf16])
@pytest.mark.parametrize("dec", [False, True])
def test_under_autocast_the_convs_get_the_fp32_swish_rounded_once(dec, half):
    m = sref.randomize(cg.ResnetBlock(in_channels=32, out_channels=64, dropout=0.0, temb_channels=0, **(dict(zq_ch=4) if dec else {})), 7).to(DEV).eval()
    rng = np.random.default_rng(51)
    x = torch.from_numpy(rng.standard_normal((4, 32, 8, 12)).astype(np.float32)).to(DEV).to(half)      # what a conv under autocast hands on
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)).to(DEV) if dec else None
    seen, hooks = _hook_inputs(m)
    with torch.no_grad(), torch.autocast("cuda", dtype=half):
        assert m.uses_kernel(x, zq)
        out = m(x, None, zq)
        a1 = m.norm1(x, zq, swish=True) if dec else m.norm1(x, swish=True)                               # the fp32-out call
        a2 = m.norm2(seen["conv1_out"], zq, swish=True) if dec else m.norm2(seen["conv1_out"], swish=True)
    for h in hooks:
        h.remove()
    assert a1.dtype == f32 and a2.dtype == f32
    assert seen["conv1"].dtype == half and torch.equal(seen["conv1"], a1.to(half)) and seen["conv1_out"].dtype == half
    assert seen["conv2"].dtype == half and torch.equal(seen["conv2"], a2.to(half))
    assert out.dtype == half
    # fp32 features under autocast (the first block behind a fp32 tensor): the reference's fp32, as before
    seen, hooks = _hook_inputs(m)
    with torch.no_grad(), torch.autocast("cuda", dtype=half):
        m(x.float(), None, zq)
    for h in hooks:
        h.remove()
    assert seen["conv1"].dtype == f32 and seen["conv2"].dtype == half


def test_with_an_active_dropout_the_convs_get_fp32():
    m = sref.randomize(cg.ResnetBlock(in_channels=32, out_channels=64, dropout=0.5, temb_channels=0), 7).to(DEV).train()
    x = torch.from_numpy(np.random.default_rng(52).standard_normal((4, 32, 8, 12)).astype(np.float32)).to(DEV).to(f16)
    seen, hooks = _hook_inputs(m)
    with torch.no_grad(), torch.autocast("cuda", dtype=f16):
        m(x, None)
        assert seen["conv1"].dtype == f32 and seen["conv2"].dtype == f32
        m.eval()
        m(x, None)
        assert seen["conv1"].dtype == f16 and seen["conv2"].dtype == f16
    for h in hooks:
        h.remove()


def _rows(what, got, want, base):
    return [(f"{what} {k}", float((got[k] - want[k]).abs().max()), float((base[k] - want[k]).abs().max())) for k in want]


def _report_and_assert(rows):
    print("  ".join(f"{k} {err / e if e else float('nan'):.2f}" for k, err, e in rows) + "   (err / E_ref)")
    for k, err, e in rows:
        assert 0 < e and err <= BAR * e, (k, err, e)


@pytest.mark.parametrize("dec", [False, True])
def test_forward_and_backward_on_the_training_kernels_against_the_torch_route(dec):
    """the same block three times: float64 on the CPU, torch's route on the device, the training kernels on the device"""
    base = sref.randomize(cg.ResnetBlock(in_channels=32, out_channels=64, dropout=0.0, temb_channels=0, **(dict(zq_ch=4) if dec else {})), 8)
    rng = np.random.default_rng(53)
    x = torch.from_numpy(rng.standard_normal((4, 32, 8, 12)).astype(np.float32))
    zq = torch.from_numpy(rng.standard_normal((4, 4, 4, 6)).astype(np.float32)) if dec else None
    go = torch.from_numpy(rng.standard_normal((4, 64, 8, 12)).astype(np.float32))
    res = {}
    for how in ("cpu64", "torch", "kernel"):
        m = copy.deepcopy(base)
        m = m.double() if how == "cpu64" else m.to(DEV)
        to = (lambda t: t.double()) if how == "cpu64" else (lambda t: t.to(DEV))
        for n in (m.norm1, m.norm2):
            n.backward_kernel = how == "kernel"
        xx = to(x).requires_grad_()
        zz = None if zq is None else to(zq)
        assert m.uses_kernel(xx, zz) == (how == "kernel")
        if how == "kernel":
            assert m.norm1.uses_backward_kernel(*((xx, zz) if dec else (xx,)))
        out = m(xx, None, zz)
        grads = torch.autograd.grad(out, [xx] + list(m.parameters()), to(go))
        res[how] = {"out": out.detach().cpu().double(), "dx": grads[0].cpu().double(),
                    **{k: g.cpu().double() for (k, _), g in zip(m.named_parameters(), grads[1:])}}
    _report_and_assert(_rows("block", res["kernel"], res["cpu64"], res["torch"]))


class _Model(torch.nn.Module):
    """what install() touches, as small as it gets, around a small encoder of the reference's shape and one decoder block"""

    def __init__(self):
        super().__init__()
        self.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
        self.encoder = gref.StandInEncoder()
        self.decoder = torch.nn.Module()
        self.decoder.block = gref.StandInBlock(64, 64, dec=True)

    def run(self, x):
        z = self.encoder(x)                                         # [B,4,8,8]
        return self.decoder.block(torch.cat([z] * 16, dim=1), None, z)


def test_install_swaps_the_expected_counts_and_the_model_agrees_with_the_unpatched_one():
    base = sref.randomize(_Model(), 9).eval()
    x = torch.from_numpy(np.random.default_rng(54).random((2, 3, 16, 16)).astype(np.float32))
    outs = {}
    for how in ("cpu64", "torch", "kernel"):
        m = copy.deepcopy(base)
        m = m.double() if how == "cpu64" else m.to(DEV)
        if how != "cpu64":
            cg.install(m, patch_group_norms=(how == "kernel"), patch_resblocks=(how == "kernel"), patch_norms=(how == "kernel"))
        count = lambda kind: sum(type(c) is kind for c in m.modules())
        if how == "kernel":
            assert (count(cg.ResnetBlock), count(norm.GroupNorm), count(norm.SpatialNorm)) == (4, 7, 2)
            assert count(torch.nn.GroupNorm) == 2 and count(gref.StandInBlock) == 0                    # the SpatialNorms' own norm layers stay
            assert [k for k in m.state_dict() if not k.startswith("quantize")] == [k for k in base.state_dict() if not k.startswith("quantize")]
        else:
            assert (count(cg.ResnetBlock), count(norm.GroupNorm), count(norm.SpatialNorm)) == (0, 0, 0)
        with torch.no_grad():
            xx = x.double() if how == "cpu64" else x.to(DEV)
            if how == "kernel":
                assert m.encoder.down[0].block[0].uses_kernel(m.encoder.conv_in(xx)) and m.decoder.block.uses_kernel(xx.new_zeros(2, 64, 8, 8), xx.new_zeros(2, 4, 8, 8))
                assert m.encoder.norm_out.uses_kernel(xx.new_zeros(2, 64, 8, 8))
            outs[how] = {"out": _Model.run(m, xx).cpu().double()}
    _report_and_assert(_rows("model", outs["kernel"], outs["cpu64"], outs["torch"]))
