"""cg.ResnetBlock without a GPU, against tests/golden/resblock.npz -- what the REAL ResnetBlocks of the reference
(vqvae_blocks.py:78-137, decoder.py:99-158) gave on the CPU (tests/golden/make_golden_resblock.py): the float64 restatement of
tests/group_norm_ref.py holds the fixture to 1e-12; the module on the CPU, built by its constructor or adopted, evaluates exactly the
reference's fp32 expression (its error against the float64 output is the fixture's own, to the bit); the state_dict keys are the
fixture's; adopt() keeps the submodules and the parameter objects; install() swaps blocks only when asked."""
import os

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import norm, resblock
import group_norm_ref as gref
import spatial_norm_ref as sref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "resblock.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files})


def load(name):
    """-> (constructor arguments, state_dict, x, zq or None, ref64, err32, keys)"""
    B, cin, cout, H, W, conv_shortcut, add_conv, dec = (int(v) for v in GOLD[name + "/shape"])
    kw = dict(in_channels=cin, out_channels=cout, conv_shortcut=bool(conv_shortcut), dropout=0.0, temb_channels=0)
    if dec:
        kw.update(zq_ch=4, add_conv=bool(add_conv))
    keys = [str(k) for k in GOLD[name + "/keys"]]
    sd = {k: torch.from_numpy(GOLD[name + "/sd/" + k]) for k in keys}
    zq = torch.from_numpy(GOLD[name + "/zq"]) if name + "/zq" in GOLD.files else None
    return kw, sd, torch.from_numpy(GOLD[name + "/x"]), zq, torch.from_numpy(GOLD[name + "/ref64"]), float(GOLD[name + "/err32"]), keys


def build(name, dtype=torch.float32):
    kw, sd, x, zq, ref64, err32, keys = load(name)
    m = cg.ResnetBlock(**kw).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return m.eval(), x, zq


def test_the_fixture_has_the_issues_cases():
    assert CASES == ["dec_add_conv", "dec_zq", "enc_conv_shortcut", "enc_nin", "enc_same"]
    shapes = {n: tuple(int(v) for v in GOLD[n + "/shape"]) for n in CASES}
    assert shapes["enc_same"][1:5] == (32, 32, 4, 6) and shapes["enc_nin"][1:5] == (32, 64, 6, 10) and shapes["enc_conv_shortcut"][5] == 1
    assert shapes["dec_zq"][1:5] == (32, 64, 4, 6) and GOLD["dec_zq/zq"].shape[2:] == (2, 3) and shapes["dec_add_conv"][6] == 1
    assert os.path.getsize(os.path.join(HERE, "golden", "resblock.npz")) < os.path.getsize(os.path.join(HERE, "golden", "spatial_norm.npz"))


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_holds_the_fixture(name):
    kw, sd, x, zq, ref64, err32, keys = load(name)
    assert float((gref.resblock64(sd, x, zq) - ref64).abs().max()) < 1e-12
    assert 0 < err32 < 1e-5


@pytest.mark.parametrize("name", CASES)
def test_the_module_on_the_cpu_is_the_references_fp32_expression(name):
    kw, sd, x, zq, ref64, err32, keys = load(name)
    m, _, _ = build(name)
    assert list(m.state_dict()) == keys
    kinds = (norm.SpatialNorm,) if "zq_ch" in kw else (norm.GroupNorm,)
    assert isinstance(m.norm1, kinds) and isinstance(m.norm2, kinds) and not m.uses_kernel(x, zq)
    with torch.no_grad():
        got = m(x, None) if zq is None else m(x, None, zq)
    assert float((got.double() - ref64).abs().max()) == err32           # the reference's own fp32 result, bit for bit
    m64, _, _ = build(name, torch.float64)
    with torch.no_grad():
        got64 = m64(x.double(), None) if zq is None else m64(x.double(), None, zq.double())
    assert torch.equal(got64, ref64)


_TheirBlock = gref.StandInBlock


@pytest.mark.parametrize("dec", [False, True])
def test_adopt_keeps_the_submodules_the_keys_and_the_arithmetic(dec):
    theirs = sref.randomize(_TheirBlock(32, 64, dec=dec, temb_channels=8), 11).eval()
    mine = cg.ResnetBlock.adopt(theirs)
    assert type(mine) is cg.ResnetBlock and list(mine.state_dict()) == list(theirs.state_dict())
    assert all(a is b for (_, a), (_, b) in zip(mine.named_parameters(), theirs.named_parameters()))
    assert mine.norm1 is theirs.norm1 and mine.conv2 is theirs.conv2 and mine.temb_proj is theirs.temb_proj and mine.dropout is theirs.dropout
    assert (mine.in_channels, mine.out_channels, mine.use_conv_shortcut, mine.training) == (32, 64, False, False)
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.standard_normal((2, 32, 4, 6)).astype(np.float32))
    temb = torch.from_numpy(rng.standard_normal((2, 8)).astype(np.float32))
    zq = torch.from_numpy(rng.standard_normal((2, 4, 2, 3)).astype(np.float32)) if dec else None
    with torch.no_grad():
        for t in (None, temb):                              # norms that are not the library's: norm, then x * sigmoid(x)
            assert torch.equal(mine(x, t, zq), theirs(x, t, zq))
    if dec:
        norm.patch_norms(mine)
    else:
        norm.patch_group_norms(mine)
    assert isinstance(mine.norm1, (norm.GroupNorm, norm.SpatialNorm)) and isinstance(mine.norm2, (norm.GroupNorm, norm.SpatialNorm))
    with torch.no_grad():                                   # the library's norms on the CPU: swish=True in the norm call, the same bits
        assert torch.equal(mine(x, temb, zq), theirs(x, temb, zq))
    with pytest.raises(TypeError, match="ResnetBlock.adopt"):
        cg.ResnetBlock.adopt(torch.nn.Conv2d(4, 4, 1))


def test_an_active_dropout_is_the_references():
    theirs = sref.randomize(_TheirBlock(32, 32, dropout=0.5), 13).train()
    mine = cg.ResnetBlock.adopt(theirs)
    x = torch.from_numpy(np.random.default_rng(14).standard_normal((2, 32, 4, 6)).astype(np.float32))
    torch.manual_seed(1)
    want = theirs(x, None)
    torch.manual_seed(1)
    assert torch.equal(mine(x, None), want) and mine.training


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
        self.encoder = torch.nn.Module()
        self.encoder.block = _TheirBlock(32, 64)
        self.decoder = torch.nn.Module()
        self.decoder.block = _TheirBlock(64, 64, dec=True)


def test_install_swaps_the_blocks_only_when_asked():
    m = _Model()
    cg.install(m)
    assert type(m.encoder.block) is _TheirBlock and type(m.decoder.block) is _TheirBlock
    assert not any(isinstance(c, (cg.ResnetBlock, norm.GroupNorm, norm.SpatialNorm)) for c in m.modules())
    keys = [k for k in m.state_dict() if not k.startswith("quantize")]
    params = {k: p for k, p in m.named_parameters() if not k.startswith("quantize")}
    cg.install(m, patch_resblocks=True)
    assert type(m.encoder.block) is cg.ResnetBlock and type(m.decoder.block) is cg.ResnetBlock
    assert type(m.encoder.block.norm1) is torch.nn.GroupNorm and type(m.decoder.block.norm1) is sref.StandIn      # the norms: their own switches
    cg.install(m, patch_resblocks=True, patch_group_norms=True, patch_norms=True)
    assert type(m.encoder.block.norm2) is norm.GroupNorm and type(m.decoder.block.norm2) is norm.SpatialNorm
    assert type(m.decoder.block.norm2.norm_layer) is torch.nn.GroupNorm
    assert [k for k in m.state_dict() if not k.startswith("quantize")] == keys
    assert all(p is params[k] for k, p in m.named_parameters() if not k.startswith("quantize"))
    assert resblock.patch_resblocks(m) == 0
