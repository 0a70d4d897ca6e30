"""CPU: the attention path (ABI 18) as far as it goes without a device.
  - the float64 restatement that the GPU tests measure against (tests/attention_ref.py), evaluated in fp32, reproduces what the real
    decoder AttnBlock handed to its proj_out (tests/golden/attn.npz, written by tests/golden/make_golden_attn.py from the real
    classes);
  - cg.AttnBlock on CPU tensors takes torch's expression and returns the real encoder block's output bit for bit; adopt() keeps the
    parameter objects and the state_dict keys of the real classes;
  - install() swaps nothing by default and every AttnBlock-shaped module with patch_attention=True;
  - the op's fake kernel gives shape and dtype; the raw call refuses CPU tensors and mismatched arguments before any pointer is taken;
  - the catalogue of infinite and saturated scores (attention_ref.SCORE_CASES): the restatement has the same NaN / +Inf / -Inf patterns
    in fp32 as in float64, the ones spelled out by index; the kernel's tile loop in torch ops (attention_ref.tiled_model) meets every
    pattern and bar of tests/test_attention_scores.py, and without the guard of a leading all -inf tile fails exactly cases a, c, g.
"""
import inspect

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import attention as att_mod_fn          # (the package exports the function under the module's name)
from control_gic_amd import _lib, norm
import attention_ref as ref
import spatial_norm_ref as norm_ref

import sys
att = sys.modules["control_gic_amd.attention"]
KEYS = ["norm.weight", "norm.bias", "q.weight", "q.bias", "k.weight", "k.bias", "v.weight", "v.bias", "proj_out.weight", "proj_out.bias"]


def test_abi_and_exports():
    assert _lib.lib().cgic_abi_version() >= 18
    assert cg.attention is att.attention and att_mod_fn is att.attention and cg.AttnBlock is att.AttnBlock
    assert {"cgic_attention", "cgic_attention_workspace_bytes", "cgic_attention_supported"} <= set(_lib.PROTOTYPES)
    assert "attention" in cg.__all__ and "AttnBlock" in cg.__all__


def test_the_restatement_in_fp32_reproduces_the_real_decoder_block(golden):
    g = golden("attn")
    q, k, v, h_ = (torch.from_numpy(g["dec/" + n]) for n in ("q", "k", "v", "h_"))
    assert q.shape == (1, 256, 8, 10) and h_.shape == q.shape
    mine = ref.restatement(q, k, v, dtype=torch.float32).reshape(h_.shape)
    assert torch.equal(mine, h_)                                # the same ops in the same order: the same bits
    r64 = ref.restatement(q, k, v)
    err = ref.max_err(h_, r64)[0]
    print(f"the class's own fp32 error against float64: {err:.3e}; torch_expr's: {ref.e_ref(r64, q, k, v):.3e}")
    assert err < 1e-5 and ref.e_ref(r64, q, k, v) == err
    l64, l32 = ref.lse64(q, k), ref.lse_torch32(q, k)
    assert l64.shape == (1, 80) and float((l32.double() - l64).abs().max()) < 1e-5


def _encoder_block(g):
    m = cg.AttnBlock(64).eval()
    assert list(m.state_dict().keys()) == [str(k) for k in g["enc/keys"]] == KEYS
    m.load_state_dict({k: torch.from_numpy(g["enc/param/" + k]) for k in KEYS})
    return m


def test_the_encoder_block_on_the_cpu_is_the_reference_bit_for_bit(golden):
    g = golden("attn")
    x, y = torch.from_numpy(g["enc/x"]), torch.from_numpy(g["enc/y"])
    m = _encoder_block(g)
    with torch.no_grad():
        assert torch.equal(m(x), y)
    theirs = ref.StandIn(64).eval()
    theirs.load_state_dict(m.state_dict())
    mine = cg.AttnBlock.adopt(theirs)
    assert all(p is q for p, q in zip(mine.parameters(), theirs.parameters())) and list(mine.state_dict().keys()) == KEYS
    assert mine.training is False
    with torch.no_grad():
        assert torch.equal(mine(x), y)
    # with a gradient: torch's expression as well, and backward() reaches the input and every parameter
    xg = x.clone().requires_grad_(True)
    out = mine(xg)
    assert torch.equal(out.detach(), y)
    out.sum().backward()
    assert xg.grad is not None and all(p.grad is not None for p in mine.parameters())


def test_the_decoder_constructor_and_keys(golden):
    g = golden("attn")
    m = cg.AttnBlock(256, 4, False)
    assert isinstance(m.norm, norm.SpatialNorm) and list(m.state_dict().keys()) == [str(k) for k in g["dec/keys"]]
    assert list(cg.AttnBlock(64, 4, True).state_dict().keys())[:4] == ["norm.norm_layer.weight", "norm.norm_layer.bias", "norm.conv.weight", "norm.conv.bias"]
    # forward(x, zq) on the CPU against the stand-in of the reference's forward on the same submodules
    theirs = ref.randomize(ref.StandIn(64, norm=norm_ref.StandIn(64)), 5).eval()
    mine = cg.AttnBlock.adopt(theirs)
    gen = torch.Generator().manual_seed(6)
    x, zq = torch.randn(2, 64, 4, 6, generator=gen), torch.randn(2, 4, 2, 3, generator=gen)
    with torch.no_grad():
        assert torch.equal(mine(x, zq), theirs(x, zq))


def test_what_has_the_reference_shape():
    assert att.has_reference_shape(ref.StandIn(64)) and att.has_reference_shape(ref.StandIn(64, norm=norm_ref.StandIn(64)))
    three = ref.StandIn(64)
    three.k = torch.nn.Conv2d(64, 64, 3, padding=1)
    narrow = ref.StandIn(64)
    narrow.proj_out = torch.nn.Conv2d(64, 32, 1)
    bare = ref.StandIn(64)
    del bare.norm
    assert not att.has_reference_shape(three) and not att.has_reference_shape(narrow) and not att.has_reference_shape(bare)
    assert not att.has_reference_shape(torch.nn.Conv2d(4, 4, 1)) and not att.has_reference_shape(norm_ref.StandIn(32))
    with pytest.raises(TypeError, match="AttnBlock.adopt"):
        cg.AttnBlock.adopt(three)


class _Model(torch.nn.Module):
    """the attribute names install() works on (model.py:42-60) around stand-ins of the reference's blocks: one encoder AttnBlock,
    two decoder AttnBlocks (each with a SpatialNorm-shaped norm) and one SpatialNorm-shaped module outside any block"""

    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Module()
        self.encoder.router_config = {"target": "somewhere.else.Router", "params": {"coarse_grain_ratio": 0.1, "medium_grain_ratio": 0.8}}
        self.encoder.mid = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 1), ref.StandIn(64))
        self.decoder = torch.nn.Module()
        self.decoder.attn = torch.nn.ModuleList([ref.StandIn(64, norm=norm_ref.StandIn(64)), ref.StandIn(32, norm=norm_ref.StandIn(32))])
        self.decoder.norm_out = norm_ref.StandIn(32)
        self.quantize = cg.VectorQuantizer(1024, 4, beta=0.25)
        self.quant_conv = torch.nn.Conv2d(4, 4, 1)
        self.post_quant_conv = torch.nn.Conv2d(4, 4, 1)

    def compress(self, x):
        raise NotImplementedError


def test_install_swaps_nothing_by_default_and_every_block_with_the_flag():
    sig = inspect.signature(cg.install)
    assert sig.parameters["patch_attention"].default is False and sig.parameters["patch_norms"].default is False
    types = lambda m: [type(x) for x in (m.encoder.mid[1], m.decoder.attn[0], m.decoder.attn[1], m.decoder.attn[0].norm, m.decoder.norm_out)]
    m = _Model()
    keys = list(m.state_dict().keys())
    cg.install(m)
    assert types(m) == [ref.StandIn, ref.StandIn, ref.StandIn, norm_ref.StandIn, norm_ref.StandIn]
    m = _Model()
    cg.install(m, patch_attention=True)
    assert types(m) == [cg.AttnBlock, cg.AttnBlock, cg.AttnBlock, norm_ref.StandIn, norm_ref.StandIn]
    assert list(m.state_dict().keys()) == keys
    assert att.patch_attention(m) == 0                          # nothing left to swap
    m = _Model()
    cg.install(m, patch_attention=True, patch_norms=True)
    assert types(m) == [cg.AttnBlock, cg.AttnBlock, cg.AttnBlock, cg.SpatialNorm, cg.SpatialNorm]
    assert type(m.decoder.attn[1].norm) is cg.SpatialNorm and type(m.encoder.mid[1].norm) is torch.nn.GroupNorm
    assert list(m.state_dict().keys()) == keys
    m = _Model()
    assert att.patch_attention(m) == 3


def test_the_ops_fake_kernel_gives_shape_and_dtype():
    with FakeTensorMode():
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            for shape in ((3, 512, 37), (2, 256, 8, 10)):
                q = torch.empty(shape, dtype=dt, device="cuda")
                got = torch.ops.cgic.attention(q, q, q, 0.0625, False)
                assert got.shape == q.shape and got.dtype == dt and got.device == q.device
                assert torch.ops.cgic.attention(q, q, q, 0.0625, True).dtype == torch.float32


def test_which_calls_reach_the_kernel():
    m = cg.AttnBlock(256).eval()
    T = lambda *s, **kw: torch.empty(*s, device="cuda", **kw)
    with FakeTensorMode():
        with torch.no_grad():
            assert m.uses_kernel(T(2, 256, 8, 10), T(2, 256, 8, 10), T(2, 256, 8, 10))
            assert m.uses_kernel(*(T(1, 512, 37, 48, dtype=torch.bfloat16),) * 3)
            assert not m.uses_kernel(*(T(2, 64, 8, 10),) * 3)                          # a width the library is not built for
            assert not m.uses_kernel(*(T(2, 256, 8, 10, dtype=torch.float64),) * 3)
            assert not m.uses_kernel(*(torch.empty(2, 256, 8, 10),) * 3)               # the CPU
        g = T(2, 256, 8, 10, requires_grad=True)
        assert not m.uses_kernel(g, T(2, 256, 8, 10), T(2, 256, 8, 10))                 # a gradient is needed
        with torch.no_grad():
            assert m.uses_kernel(g, g, g)
    assert att.supported(torch.float32, torch.float32, 1, 256, 1) and not att.supported(torch.float32, torch.float16, 1, 256, 1)
    assert not att.supported(torch.float64, torch.float64, 1, 256, 1)


def test_the_raw_call_refuses_before_it_takes_a_pointer():
    q = torch.zeros(1, 256, 6)
    with pytest.raises(Exception, match="(?i)cpu|device|cuda"):
        cg.attention(q, q, q)
    with pytest.raises(Exception, match="(?i)cpu|device|cuda"):
        cg.attention(q.half(), q.half(), q.half(), lse=True)
    with FakeTensorMode():
        T = lambda *s, **kw: torch.empty(*s, device="cuda", **kw)
        q = T(2, 256, 6)
        with pytest.raises(TypeError, match="expected fp32, fp16 or bf16"):
            cg.attention(T(2, 256, 6, dtype=torch.float64), q, q)
        with pytest.raises(TypeError, match="expected fp32, fp16 or bf16"):
            cg.attention(T(256, 6), T(256, 6), T(256, 6))
        with pytest.raises(ValueError, match="attention: k"):
            cg.attention(q, T(2, 256, 7), q)
        with pytest.raises(ValueError, match="attention: v"):
            cg.attention(q, q, T(2, 256, 6, dtype=torch.float16))
        with pytest.raises(ValueError, match="attention: out"):
            cg.attention(q, q, q, out=T(2, 256, 7))
        with pytest.raises(TypeError, match="out_dtype"):
            cg.attention(q, q, q, out=T(2, 256, 6), out_dtype=torch.float16)
        with pytest.raises(TypeError, match="result type"):
            cg.attention(q, q, q, out_dtype=torch.float16)
        with pytest.raises(TypeError, match="result type"):
            cg.attention(q.half(), q.half(), q.half(), out_dtype=torch.bfloat16)


# ---- infinite and saturated scores: the catalogue of tests/attention_ref.py without a device
_score = {}
_ids = [f"{name}-C{C}-{str(dt).split('.')[1]}" for name, C, dt in ref.SCORE_PARAMS]


def score_case(name, C, dtype):
    """(the built case, its references on the CPU): made once, shared, never changed"""
    key = (name, C, dtype)
    if key not in _score:
        c = ref.build_case(name, C, dtype)
        _score[key] = (c, ref.case_refs(c))
    return _score[key]


@pytest.mark.parametrize("name,C,dtype", ref.SCORE_PARAMS, ids=_ids)
def test_float64_is_a_fair_reference_on_the_score_catalogue(name, C, dtype):
    """the restatement in fp32 puts NaN, +Inf and -Inf where the restatement in float64 puts them, and both where the case spells
    them out by index: on these inputs the patterns do not depend on the precision of the reference"""
    c, r = score_case(name, C, dtype)
    r32 = ref.restatement(c.q, c.k, c.v, c.scale, dtype=torch.float32)
    assert ref.same_patterns(r32, r.r64)
    assert ref.same_patterns(r.r64, c.expect) and ref.same_patterns(r32, c.expect)
    assert bool(torch.isfinite(r.r64[1]).all())                                  # image 1 is clean
    if name == "n":
        print(f"one-hot rows: the largest runner-up weight in float64 is {r.runner_up:.3e}")
        assert r.runner_up < 2.0 ** -60


@pytest.mark.parametrize("name,C,dtype", ref.SCORE_PARAMS, ids=_ids)
def test_the_tile_loop_with_the_guard_meets_every_pattern_and_bar(name, C, dtype):
    """the kernel's algorithm (attention_ref.tiled_model, guard=True) passes what tests/test_attention_scores.py asks of the kernel:
    the bars are conditions the algorithm can meet"""
    c, r = score_case(name, C, dtype)
    out, lse = ref.tiled_model(c.q, c.k, c.v, c.scale, guard=True)
    ref.judge(c, r, out, lse, f"tile loop, {name} C{C} {dtype}")


def test_without_the_guard_the_tile_loop_fails_exactly_the_leading_inf_tile_cases():
    """guard=False is the kernel's arithmetic before the fix: exp2(-inf - -inf) in a leading tile whose scores are all -inf.  It must
    fail the pattern check on cases a, c and g at every width and type, and on no other case: the catalogue catches this class of
    error, and nothing else in it depends on the guard"""
    failed, passed = set(), set()
    for name, C, dtype in ref.SCORE_PARAMS:
        c, r = score_case(name, C, dtype)
        out, lse = ref.tiled_model(c.q, c.k, c.v, c.scale, guard=False)
        ok = ref.same_patterns(out, c.expect)
        if not ok:
            nan = int(torch.isnan(out[0]).any(dim=0).sum())
            print(f"{name} C{C} {dtype}: NaN at {nan} of {c.N} queries of image 0, the reference at {int(c.expect[0][0].any(dim=0).sum())}")
        (passed if ok else failed).add(name)
    assert failed == set(ref.LEADING_INF_TILE) and not (failed & passed)
