"""The CPU side of the multi-tensor EMA (control_gic_amd/ema.py, csrc/cgic_ema.hip), no GPU:
  - tests/ema_ref.py, the torch restatement the GPU tests compare with, against tests/golden/ema.npz, which the REAL LitEma wrote
    (tests/golden/make_golden_ema.py): bit for bit, every step, with and without use_num_upates and across the crossing at 0.9999;
  - the ABI: the header declares the five entry points, the library exports them, _lib.PROTOTYPES binds them with the declared
    argument counts, ABI >= 22; calls the plan refuses are refused without a device (made-up addresses, never dereferenced);
  - the op's schema, its fake kernel, and every refusal of EmaPlan and of the op under FakeTensorMode on fake "cuda" tensors;
  - cg.LitEma: the recorded state_dict keys, load_state_dict of the recorded state, the ValueError, adopt;
  - install(patch_ema=...): off by default and then the attributes are left alone; with it, which are swapped, on the same buffers.
"""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib, ema
import ema_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ema.npz"))
RUNS = {"plain": False, "counted": True, "cross": True}
STEPS = 5
ENTRY_POINTS = {"cgic_ema_plan_create": 3, "cgic_ema_plan_destroy": 1, "cgic_ema_plan_info": 2, "cgic_ema_update": 4, "cgic_ema_copy": 4}


# ---------------------------------------------------------------------------- the restatement against the real class
@pytest.mark.parametrize("tag", RUNS)
def test_the_restatement_is_the_real_class_bit_for_bit(tag):
    names = [str(k) for k in GOLDEN[tag + "/names"]]
    trainable = [k for k, t in zip(names, GOLDEN[tag + "/trainable"]) if t]
    assert "frozen" in names and "frozen" not in trainable and GOLDEN[tag + "/init/head.bias"].shape == (1,)
    shadows = [torch.from_numpy(GOLDEN[f"{tag}/init/{k}"]) for k in trainable]
    n = int(GOLDEN[tag + "/start"])
    assert (n >= 0) == RUNS[tag]
    for step in range(STEPS):
        params = [torch.from_numpy(GOLDEN[f"{tag}/param{step}/{k}"]) for k in trainable]
        shadows, n2 = eref.update(shadows, params, 0.9999, n if RUNS[tag] else None)
        n = n2 if RUNS[tag] else -1
        assert n == int(GOLDEN[f"{tag}/num_updates{step}"])
        for k, s in zip(trainable, shadows):
            assert torch.equal(eref.bits(s), eref.bits(torch.from_numpy(GOLDEN[f"{tag}/shadow{step}/{k}"]))), (tag, step, k)
    assert int(GOLDEN["cross/start"]) == 89988 and int(GOLDEN["cross/num_updates4"]) == 89993 and int(GOLDEN["counted/num_updates0"]) == 1


def test_the_recorded_model_shapes():
    numel, shape, owner = GOLDEN["model/numel"], GOLDEN["model/shape"], GOLDEN["model/owner"]
    assert len(numel) == 655 and int(numel.sum()) == 130358967 and [int((owner == i).sum()) for i in range(5)] == [204, 446, 1, 2, 2]
    assert [str(p) for p in GOLDEN["model/parts"]] == ["encoder", "decoder", "quantize", "quant_conv", "post_quant_conv"]
    assert np.array_equal(np.where(shape < 0, 1, shape).prod(axis=1), numel) and int(np.median(numel)) == 512


# ---------------------------------------------------------------------------- the ABI
def test_header_library_and_prototypes_agree_on_the_five_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cgic_hip.h")).read()
    assert int(re.search(r"^#define\s+CGIC_ABI_VERSION\s+(\d+)", hdr, re.M).group(1)) >= 22
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    l = ctypes.CDLL(cg.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, code, re.S)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(l, name), f"{name} is not exported"
    assert _lib.lib().cgic_abi_version() >= 22
    assert ctypes.sizeof(_lib.EmaEntry) == 24 and "typedef struct cgic_ema_entry" in code


def test_the_library_refuses_what_the_plan_refuses_without_a_device():
    """a refused create allocates and uploads nothing: it can be made with made-up addresses"""
    def refused(text, entries, n=None):
        arr = (_lib.EmaEntry * max(len(entries), 1))()
        for e, (s, p, k) in zip(arr, entries):
            e.shadow, e.param, e.n = s, p, k
        h = ctypes.c_void_p()
        with pytest.raises(cg.CgicError) as got:
            _lib.call("cgic_ema_plan_create", arr, len(entries) if n is None else n, ctypes.byref(h))
        assert got.value.code == _lib.ERR_INVALID and text in str(got.value) and not h.value, str(got.value)

    S, P = 1 << 36, 2 << 36
    refused("ema_plan: entry 1 has a NULL shadow with 5 elements", [(S, P, 3), (None, P + 64, 5)])
    refused("ema_plan: the param of entry 0 is not aligned to its 4-byte element", [(S, P + 2, 3)])
    refused("ema_plan: entry 0 has -1 elements", [(S, P, -1)])
    refused("ema_plan: -1 entries", [], n=-1)
    refused("ema_plan: more than 2^31 - 1 chunks of 4096 elements", [(S, P, 1 << 43)])
    for name, args in (("cgic_ema_update", (None, None, None, None)), ("cgic_ema_copy", (None, 0, None, None)), ("cgic_ema_plan_info", (None, None))):
        with pytest.raises(cg.CgicError, match="NULL"):
            _lib.call(name, *args)
    _lib.lib().cgic_ema_plan_destroy(None)                      # a no-op


# ---------------------------------------------------------------------------- the op and EmaPlan under FakeTensorMode
def test_the_ops_schema_and_fake_kernel():
    schema = torch.ops.cgic.ema_update.default._schema
    assert str(schema) == "cgic::ema_update(Tensor(a0!)[] shadows, Tensor[] params, Tensor decay, Tensor(a3!)? num_updates) -> ()"
    written = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert written == {"shadows", "num_updates"} and len(schema.returns) == 0
    with FakeTensorMode():
        s, p = [torch.empty(3, 5, device="cuda"), torch.empty((), device="cuda")], [torch.empty(3, 5, device="cuda"), torch.empty((), device="cuda")]
        decay, n = torch.empty((), device="cuda"), torch.empty((), device="cuda", dtype=torch.int32)
        assert torch.ops.cgic.ema_update(s, p, decay, n) is None
        assert torch.ops.cgic.ema_update(s, p, decay, None) is None
        assert torch.ops.cgic.ema_update([], [], decay, n) is None


REFUSALS = [
    ("count", ValueError, "{who}: 2 shadows for 1 params"),
    ("cpu", RuntimeError, "control_gic_amd ops run on an MI355X (HIP) device only; got a CPU tensor. "
                          "There is deliberately no CPU fallback -- the CPU oracle lives in oracle/ and is test-only."),
    ("half", TypeError, "{who}: pair 1 is torch.float16 / torch.float32; the kernel takes torch.float32 (LitEma updates other pairs with torch's expression)"),
    ("shape", ValueError, "{who}: pair 1: shadow (3, 5), param (5, 3)"),
    ("strides", ValueError, "{who}: pair 1: shadow strides (5, 1), param strides (1, 3) of shape (3, 5); the kernel takes contiguous tensors"),
]
SCALAR_REFUSALS = [
    ("decay-half", TypeError, "{who}: decay torch.float16 () on cuda:0; expected one torch.float32 element on cuda:0 (LitEma's buffer: the value is read on the device)"),
    ("decay-two", TypeError, "{who}: decay torch.float32 (2,) on cuda:0; expected one torch.float32 element on cuda:0 (LitEma's buffer: the value is read on the device)"),
    ("decay-cpu", TypeError, "{who}: decay torch.float32 () on cpu; expected one torch.float32 element on cuda:0 (LitEma's buffer: the value is read on the device)"),
    ("count-int64", TypeError, "{who}: num_updates torch.int64 () on cuda:0; expected one torch.int32 element on cuda:0 (LitEma's buffer: the value is read on the device)"),
]


def _fake_case(kind):
    T = lambda *s, **kw: torch.empty(*s, device=kw.pop("device", "cuda:0"), **kw)
    s, p = [T(4), T(3, 5)], [T(4), T(3, 5)]
    decay, n = T(()), T((), dtype=torch.int32)
    if kind == "count":
        p = p[:1]
    elif kind == "cpu":
        p[1] = T(3, 5, device="cpu")
    elif kind == "half":
        s[1] = T(3, 5, dtype=torch.float16)
    elif kind == "shape":
        p[1] = T(5, 3)
    elif kind == "strides":
        p[1] = T(5, 3).t()
    elif kind == "decay-half":
        decay = T((), dtype=torch.float16)
    elif kind == "decay-two":
        decay = T(2)
    elif kind == "decay-cpu":
        decay = T((), device="cpu")
    elif kind == "count-int64":
        n = T((), dtype=torch.int64)
    return s, p, decay, n


@pytest.mark.parametrize("kind,exc,text", REFUSALS + SCALAR_REFUSALS, ids=[r[0] for r in REFUSALS + SCALAR_REFUSALS])
def test_the_op_refuses_with_the_full_message(kind, exc, text):
    """under FakeTensorMode a data_ptr() would raise another error: the message comes first"""
    with FakeTensorMode():
        s, p, decay, n = _fake_case(kind)
        with pytest.raises(exc) as got:
            torch.ops.cgic.ema_update(s, p, decay, n)
        assert text.format(who="ema_update") in str(got.value)
        with pytest.raises(exc) as got:
            ema._ema_update(s, p, decay, n)                      # the binding itself: the same checks before any pointer
        assert text.format(who="ema_update") in str(got.value)


@pytest.mark.parametrize("kind,exc,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_ema_plan_refuses_with_the_full_message(kind, exc, text):
    with FakeTensorMode():
        s, p, _, _ = _fake_case(kind)
        with pytest.raises(exc) as got:
            cg.EmaPlan(s, p)
        assert text.format(who="EmaPlan") in str(got.value)


def test_two_devices_in_one_plan_are_refused():
    with FakeTensorMode():
        s = [torch.empty(4, device="cuda:0"), torch.empty(4, device="cuda:1")]
        with pytest.raises(ValueError) as got:
            cg.EmaPlan(s, s)
        assert "EmaPlan: pair 1 is on cuda:1 / cuda:1; pair 0 is on cuda:0 (one plan, one device)" in str(got.value)


# ---------------------------------------------------------------------------- the module
@pytest.mark.parametrize("tag", RUNS)
def test_litema_has_the_recorded_keys_and_loads_the_recorded_state(tag):
    m = eref.Small().load(GOLDEN, tag + "/init")
    e = cg.LitEma(m, 0.9999, use_num_upates=RUNS[tag])
    keys = [str(k) for k in GOLDEN[tag + "/keys"]]
    assert list(e.state_dict().keys()) == keys and keys[:2] == ["decay", "num_updates"] and "convweight" in keys and "frozen" not in keys
    assert e.m_name2s_name == {k: k.replace(".", "") for k, p in m.named_parameters() if p.requires_grad} and e.collected_params == []
    assert e.decay.dtype == torch.float32 and e.num_updates.dtype == torch.int32 and int(e.num_updates) == (0 if RUNS[tag] else -1)
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(e._buffers[e.m_name2s_name[k]], p) and e._buffers[e.m_name2s_name[k]] is not p
    sd = {k: torch.from_numpy(GOLDEN[f"{tag}/sd/{k}"]) for k in keys}
    assert e.load_state_dict(sd, strict=True).missing_keys == []
    assert int(e.num_updates) == int(GOLDEN[tag + "/num_updates4"])
    assert torch.equal(eref.bits(e.convweight), eref.bits(torch.from_numpy(GOLDEN[tag + "/shadow4/conv.weight"])))
    assert list(copy.deepcopy(e).state_dict().keys()) == keys


def test_litema_refuses_a_decay_outside_0_1():
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="Decay must be between 0 and 1"):
            cg.LitEma(eref.Small(), bad)
    cg.LitEma(eref.Small(), 0.0), cg.LitEma(eref.Small(), 1.0)
    sig = inspect.signature(cg.LitEma.__init__)
    assert list(sig.parameters) == ["self", "model", "decay", "use_num_upates"] and sig.parameters["decay"].default == 0.9999 \
        and sig.parameters["use_num_upates"].default is False
    for name in ("forward", "copy_to", "store", "restore", "adopt"):
        assert callable(getattr(cg.LitEma, name))
    assert cg.ema is ema and cg.EmaPlan is ema.EmaPlan


def test_litema_on_the_cpu_is_the_references_expression():
    """pairs the kernel does not take -- here all of them: CPU tensors -- are updated by torch's expression, counter included"""
    for tag in RUNS:
        m = eref.Small().load(GOLDEN, tag + "/init")
        e = cg.LitEma(m, 0.9999, use_num_upates=RUNS[tag])
        e.num_updates.fill_(int(GOLDEN[tag + "/start"]))
        for step in range(STEPS):
            e(m.load(GOLDEN, f"{tag}/param{step}"))
            assert int(e.num_updates) == int(GOLDEN[f"{tag}/num_updates{step}"])
            for k, sname in e.m_name2s_name.items():
                assert torch.equal(eref.bits(e._buffers[sname]), eref.bits(torch.from_numpy(GOLDEN[f"{tag}/shadow{step}/{k}"]))), (tag, step, k)
        before = {k: p.detach().clone() for k, p in m.named_parameters()}
        e.store(m.parameters())
        e.copy_to(m)
        assert torch.equal(m.conv.weight, e.convweight) and not torch.equal(m.conv.weight, before["conv.weight"]) and torch.equal(m.frozen, before["frozen"])
        e.restore(m.parameters())
        assert all(torch.equal(eref.bits(p), eref.bits(before[k])) for k, p in m.named_parameters())


def test_adopt_takes_over_the_buffers():
    m = eref.Small()
    theirs = eref.StandIn(m, 0.99, use_num_upates=True)
    mine = cg.LitEma.adopt(theirs)
    assert isinstance(mine, cg.LitEma) and list(mine.state_dict().keys()) == list(theirs.state_dict().keys())
    assert all(mine._buffers[k] is theirs._buffers[k] for k in theirs._buffers) and mine.m_name2s_name is theirs.m_name2s_name
    with pytest.raises(TypeError, match="LitEma.adopt: Linear has not the reference's m_name2s_name / decay / num_updates"):
        cg.LitEma.adopt(torch.nn.Linear(2, 2))


# ---------------------------------------------------------------------------- install()
def _model():
    model = torch.nn.Module()
    model.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
    model.encoder = eref.Small()
    model.decoder = eref.Small()
    model.quant_conv = torch.nn.Conv2d(4, 4, 1)
    model.post_quant_conv = torch.nn.Conv2d(4, 4, 1)
    for name in ("encoder", "decoder", "quantize", "quant_conv", "post_quant_conv"):
        setattr(model, "ema_" + name, eref.StandIn(getattr(model, name)))
    model.not_an_ema = torch.nn.Linear(2, 2)
    return model


EMA_NAMES = ["ema_encoder", "ema_decoder", "ema_quantize", "ema_quant_conv", "ema_post_quant_conv"]


def test_install_leaves_the_ema_modules_alone_unless_asked():
    assert inspect.signature(cg.install).parameters["patch_ema"].default is False
    model = _model()
    before = {n: getattr(model, n) for n in EMA_NAMES}
    cg.install(model)
    assert all(getattr(model, n) is before[n] and type(before[n]) is eref.StandIn for n in EMA_NAMES)


def test_install_patch_ema_swaps_the_five_on_their_own_buffers():
    model = _model()
    before = {n: getattr(model, n) for n in EMA_NAMES}
    keys = list(model.state_dict().keys())
    cg.install(model, patch_ema=True)
    for n in EMA_NAMES:
        new = getattr(model, n)
        assert type(new) is cg.LitEma and all(new._buffers[k] is before[n]._buffers[k] for k in before[n]._buffers)
        assert list(new._buffers) == list(before[n]._buffers)
    assert type(model.not_an_ema) is torch.nn.Linear and type(model.encoder) is eref.Small
    assert [k for k in model.state_dict().keys() if k.startswith("ema_")] == [k for k in keys if k.startswith("ema_")]
    # the adopted ema_quantize keeps working with the VectorQuantize2 install swapped in: names are matched against the module
    # forward is called with, and its usage counters are not trainable
    assert isinstance(model.quantize, cg.VectorQuantize2) and list(model.ema_quantize.m_name2s_name) == ["embedding.weight"]
    assert [k for k, p in model.quantize.named_parameters() if p.requires_grad] == ["embedding.weight"]
    model.quantize.embedding.weight.data.add_(1.0)
    want = eref.step(model.ema_quantize.embeddingweight.clone(), model.quantize.embedding.weight.detach(), eref.one_minus_decay(0.9999))
    model.ema_quantize(model.quantize)
    assert torch.equal(eref.bits(model.ema_quantize.embeddingweight), eref.bits(want))
    assert ema.patch_ema(model) == []                           # nothing left to swap
