"""The CPU side of the multi-tensor Adam (control_gic_amd/adam.py, csrc/cgic_adam.hip), no GPU:
  - tests/adam_ref.py, the restatement the GPU tests compare with bit for bit, against the REAL torch.optim.Adam on the CPU.  They are
    not bit-identical -- torch's CPU kernels fuse a multiply-add in addcmul_ -- so the bar is the project's usual one: against a float64
    restatement of the same steps the error of adam_ref is at most 4x torch's own, per tensor;
  - the ABI: the header declares the four entry points, the library exports them, _lib.PROTOTYPES binds them with the declared argument
    counts, ABI 23; calls the plan refuses are refused without a device (made-up addresses, never dereferenced);
  - the op's schema, its fake kernel and the refusals of AdamPlan and the op under FakeTensorMode;
  - cg.Adam without a device: every parameter is on torch's path and the result is torch.optim.Adam's; the state_dict keys;
    load_state_dict from a plain torch.optim.Adam's dict and back; the clip of the fallback;
  - install(patch_optimizers=...): off by default; with it configure_optimizers returns cg.Adam on the same groups and defaults."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import _lib, adam
import adam_ref as aref
import ema_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"cgic_adam_plan_create": 6, "cgic_adam_plan_destroy": 1, "cgic_adam_plan_info": 2, "cgic_adam_step": 4}


# ---------------------------------------------------------------------------- the restatement against the real optimiser
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_the_restatement_against_torch_adam_and_float64(weight_decay):
    """8 steps of 100 003 elements, gradients spanning 1e-6 .. 1e2 in size, lr 5e-5, betas (0.5, 0.9): the largest error of adam_ref
    against the float64 chain is at most 4x that of torch.optim.Adam(foreach=False), for param, exp_avg and exp_avg_sq"""
    n, steps, lr, betas = 100003, 8, 5e-5, (0.5, 0.9)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32) for _ in range(steps)]
    w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([w], lr=lr, betas=betas, weight_decay=weight_decay, foreach=False)
    P, M, V, T = [p0.copy()], [np.zeros(n, np.float32)], [np.zeros(n, np.float32)], np.zeros(1, np.float32)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        w.grad = torch.from_numpy(g.copy())
        opt.step()
        P, M, V, T, _ = aref.step(P, [g], M, V, T, lr, betas, weight_decay=weight_decay)
        p64, m64, v64 = aref.step64(p64, g, m64, v64, t, lr, betas, weight_decay=weight_decay)
    assert T[0] == steps == float(opt.state[w]["step"])
    theirs = (w.detach().numpy(), opt.state[w]["exp_avg"].numpy(), opt.state[w]["exp_avg_sq"].numpy())
    for name, mine, torchs, exact in zip(("param", "exp_avg", "exp_avg_sq"), (P[0], M[0], V[0]), theirs, (p64, m64, v64)):
        err_mine, err_torch = np.abs(mine.astype(np.float64) - exact).max(), np.abs(torchs.astype(np.float64) - exact).max()
        differ = int((aref.bits(mine) != aref.bits(torchs)).sum())
        print(f"weight_decay {weight_decay} {name}: adam_ref {err_mine:.3e}, torch {err_torch:.3e}, ratio {err_mine / err_torch:.3f}, elements that differ {differ} of {n}")
        assert err_torch > 0 and err_mine <= 4 * err_torch, (name, err_mine, err_torch)


def test_the_float64_chain_uses_pythons_power():
    p, m, v = aref.step64([1.0], [0.5], [0.0], [0.0], 1, 1e-3, (0.9, 0.999))
    assert m[0] == (1.0 - 0.9) * 0.5 and v[0] == (1.0 - 0.999) * 0.25 and abs(p[0] - (1.0 - 1e-3)) < 1e-9


# ---------------------------------------------------------------------------- the ABI
def test_header_library_and_prototypes_agree_on_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "cgic_hip.h")).read()
    assert int(re.search(r"^#define\s+CGIC_ABI_VERSION\s+(\d+)", hdr, re.M).group(1)) >= 23
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    l = ctypes.CDLL(cg.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, code, re.S)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert hasattr(l, name), f"{name} is not exported"
    assert _lib.lib().cgic_abi_version() >= 23
    assert ctypes.sizeof(_lib.AdamEntry) == 48 and ctypes.sizeof(_lib.AdamEmaGroup) == 16 and ctypes.sizeof(_lib.AdamHyper) == 64
    for name in ("cgic_adam_entry", "cgic_adam_ema_group", "cgic_adam_hyper"):
        assert "typedef struct " + name in code


def test_the_library_refuses_what_the_plan_refuses_without_a_device():
    """a refused create allocates and uploads nothing: it can be made with made-up addresses"""
    P, M, V, S, T, D = (k << 36 for k in range(1, 7))

    def refused(text, entries, groups=(), n=None, ngroups=None, steps=T):
        arr = (_lib.AdamEntry * max(len(entries), 1))()
        for e, (p, m, v, s, k, g) in zip(arr, entries):
            e.param, e.exp_avg, e.exp_avg_sq, e.shadow, e.n, e.ema_group = p, m, v, s, k, g
        gr = (_lib.AdamEmaGroup * max(len(groups), 1))()
        for e, (d, c) in zip(gr, groups):
            e.decay, e.num_updates = d, c
        h = ctypes.c_void_p()
        with pytest.raises(cg.CgicError) as got:
            _lib.call("cgic_adam_plan_create", arr, len(entries) if n is None else n, gr, len(groups) if ngroups is None else ngroups, steps, ctypes.byref(h))
        assert got.value.code == _lib.ERR_INVALID and text in str(got.value) and not h.value, str(got.value)

    refused("adam_plan: entry 1 has a NULL exp_avg with 5 elements", [(P, M, V, None, 3, -1), (P + 64, None, V + 64, None, 5, -1)])
    refused("adam_plan: the exp_avg_sq of entry 0 is not aligned to its 4-byte element", [(P, M, V + 2, None, 3, -1)])
    refused("adam_plan: entry 0 has -1 elements", [(P, M, V, None, -1, -1)])
    refused("adam_plan: entry 0 names EMA group 0 of 0 (-1: no shadow)", [(P, M, V, S, 3, 0)])
    refused("adam_plan: entry 0 has a NULL shadow with 3 elements in EMA group 0", [(P, M, V, None, 3, 0)], [(D, None)])
    refused("adam_plan: 17 EMA groups (0 .. 16)", [], [(D, None)], ngroups=17)
    refused("adam_plan: -1 entries", [], n=-1)
    refused("adam_plan: NULL step counts with 1 entries", [(P, M, V, None, 3, -1)], steps=None)
    refused("adam_plan: more than 2^31 - 1 chunks of 4096 elements", [(P, M, V, None, 1 << 43, -1)])
    for name, args in (("cgic_adam_step", (None, None, None, None)), ("cgic_adam_plan_info", (None, None))):
        with pytest.raises(cg.CgicError, match="NULL"):
            _lib.call(name, *args)
    _lib.lib().cgic_adam_plan_destroy(None)                     # a no-op


# ---------------------------------------------------------------------------- the op and AdamPlan under FakeTensorMode
def test_the_ops_schema_and_fake_kernel():
    schema = torch.ops.cgic.adam_step.default._schema
    written = {a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write}
    assert written == {"params", "exp_avgs", "exp_avg_sqs", "steps", "shadows", "num_updates"} and len(schema.returns) == 0
    assert [a.name for a in schema.arguments] == ["params", "grads", "exp_avgs", "exp_avg_sqs", "steps", "lr", "beta1", "beta2", "eps", "weight_decay",
                                                  "clip_value", "lr_tensor", "shadows", "decay", "num_updates"]
    with FakeTensorMode():
        T = lambda *s, **kw: torch.empty(*s, device="cuda:0", **kw)
        p, m, v, s = ([T(3, 5), T(())] for _ in range(4))
        steps, decay, n, lr = T(2), T(()), T((), dtype=torch.int32), T(())
        assert torch.ops.cgic.adam_step(p, [T(3, 5), None], m, v, steps, 5e-5, 0.5, 0.9, 1e-8, 0.0, 1.0, None, [], None, None) is None
        assert torch.ops.cgic.adam_step(p, [None, None], m, v, steps, 0.0, 0.5, 0.9, 1e-8, 0.01, None, lr, s, decay, n) is None
        assert torch.ops.cgic.adam_step([], [], [], [], T(0), 5e-5, 0.5, 0.9, 1e-8, 0.0, None, None, [], None, None) is None


def _fake_lists():
    T = lambda *s, **kw: torch.empty(*s, device=kw.pop("device", "cuda:0"), **kw)
    return T, [T(4), T(3, 5)], [T(4), T(3, 5)], [T(4), T(3, 5)], T(2)


REFUSALS = [
    ("count", ValueError, "{who}: 2 params, 1 exp_avgs, 2 exp_avg_sqs"),
    ("cpu", RuntimeError, "control_gic_amd ops run on an MI355X (HIP) device only; got a CPU tensor."),
    ("half", TypeError, "{who}: the exp_avg of entry 1 is torch.float16; the kernel takes torch.float32 (cg.Adam updates other parameters with torch's implementation)"),
    ("shape", ValueError, "{who}: entry 1: param (3, 5), exp_avg_sq (5, 3)"),
    ("strides", ValueError, "{who}: the param of entry 1 has strides (1, 3) of shape (3, 5); the kernel takes contiguous tensors"),
    ("device", ValueError, "{who}: the exp_avg of entry 0 is on cuda:1; the step counts are on cuda:0 (one plan, one device)"),
    ("steps-size", TypeError, "{who}: steps torch.float32 (3,) on cuda:0; expected contiguous torch.float32 [2], one step count per entry"),
    ("steps-int", TypeError, "{who}: steps torch.int64 (2,) on cuda:0; expected contiguous torch.float32 [2], one step count per entry"),
]


def _refusal_case(kind):
    T, p, m, v, steps = _fake_lists()
    if kind == "count":
        m = m[:1]
    elif kind == "cpu":
        v[1] = T(3, 5, device="cpu")
    elif kind == "half":
        m[1] = T(3, 5, dtype=torch.float16)
    elif kind == "shape":
        v[1] = T(5, 3)
    elif kind == "strides":
        p[1] = T(5, 3).t()
    elif kind == "device":
        m[0] = T(4, device="cuda:1")
    elif kind == "steps-size":
        steps = T(3)
    elif kind == "steps-int":
        steps = T(2, dtype=torch.int64)
    return p, m, v, steps


@pytest.mark.parametrize("kind,exc,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_plan_and_the_op_refuse_with_the_full_message(kind, exc, text):
    """under FakeTensorMode a data_ptr() would raise another error: the message comes first"""
    with FakeTensorMode():
        p, m, v, steps = _refusal_case(kind)
        with pytest.raises(exc) as got:
            cg.AdamPlan(p, m, v, steps)
        assert text.format(who="AdamPlan") in str(got.value)
        with pytest.raises(exc) as got:
            torch.ops.cgic.adam_step(p, [None, None], m, v, steps, 5e-5, 0.5, 0.9, 1e-8, 0.0, None, None, [], None, None)
        assert text.format(who="adam_step") in str(got.value)


def test_shadows_groups_and_hyperparameters_are_refused():
    with FakeTensorMode():
        T, p, m, v, steps = _fake_lists()
        decay, n = T(()), T((), dtype=torch.int32)
        with pytest.raises(ValueError, match=r"AdamPlan: 1 shadows for 2 params \(None where a parameter has none\)"):
            cg.AdamPlan(p, m, v, steps, [T(4)], None, [(decay, n)])
        with pytest.raises(ValueError, match=r"AdamPlan: entry 1 has a shadow and EMA group 1 of 1 \(-1: none\)"):
            cg.AdamPlan(p, m, v, steps, [T(4), T(3, 5)], [0, 1], [(decay, n)])
        with pytest.raises(ValueError, match=r"AdamPlan: entry 0 has no shadow and EMA group 0 of 1"):
            cg.AdamPlan(p, m, v, steps, [None, T(3, 5)], [0, 0], [(decay, n)])
        with pytest.raises(ValueError, match="AdamPlan: 17 EMA groups; a plan takes up to 16"):
            cg.AdamPlan(p, m, v, steps, None, None, [(decay, n)] * 17)
        with pytest.raises(TypeError, match="AdamPlan: num_updates of EMA group 0 torch.int64"):
            cg.AdamPlan(p, m, v, steps, [T(4), T(3, 5)], None, [(decay, T((), dtype=torch.int64))])
        with pytest.raises(ValueError, match="adam_step: shadows and decay come together"):
            torch.ops.cgic.adam_step(p, [None, None], m, v, steps, 5e-5, 0.5, 0.9, 1e-8, 0.0, None, None, [T(4), T(3, 5)], None, None)
        for args, text in (((-1.0, 0.5, 0.9, 1e-8, 0.0, None), "Invalid learning rate: -1.0"), ((1e-3, 1.0, 0.9, 1e-8, 0.0, None), "Invalid beta parameter at index 0: 1.0"),
                           ((1e-3, 0.5, -0.1, 1e-8, 0.0, None), "Invalid beta parameter at index 1: -0.1"), ((1e-3, 0.5, 0.9, -1.0, 0.0, None), "Invalid epsilon value: -1.0"),
                           ((1e-3, 0.5, 0.9, 1e-8, -0.5, None), "Invalid weight_decay value: -0.5"), ((1e-3, 0.5, 0.9, 1e-8, 0.0, -1.0), "Invalid clip_value: -1.0"),
                           ((1e-3, 0.5, 0.9, 1e-8, 0.0, float("nan")), "Invalid clip_value: nan")):
            with pytest.raises(ValueError) as got:
                torch.ops.cgic.adam_step(p, [None, None], m, v, steps, *args, None, [], None, None)
            assert text in str(got.value)
        with pytest.raises(TypeError, match="adam_step: lr torch.float16"):
            torch.ops.cgic.adam_step(p, [None, None], m, v, steps, 0.0, 0.5, 0.9, 1e-8, 0.0, None, T((), dtype=torch.float16), [], None, None)


# ---------------------------------------------------------------------------- cg.Adam without a device
class Toy(torch.nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(33, generator=g))
        self.b = torch.nn.Parameter(torch.randn(4, 9, generator=g))
        self.unused = torch.nn.Parameter(torch.randn(3, generator=g))

    def loss(self, k):
        return (self.a * (k + 1)).sin().sum() + (self.b ** 2).sum() * 0.1 * (k + 1)

    def configure_optimizers(self):
        return [torch.optim.Adam([self.a, self.b], lr=5e-5, betas=(0.5, 0.9)), torch.optim.SGD([self.unused], lr=0.1)], []


def _run(model, opt, steps, start=0):
    for k in range(start, start + steps):
        opt.zero_grad(set_to_none=True)
        model.loss(k).backward()
        opt.step()


def test_on_the_cpu_every_parameter_takes_torchs_path_and_the_result_is_torchs():
    sig = inspect.signature(cg.Adam.__init__)
    assert list(sig.parameters)[:6] == ["self", "params", "lr", "betas", "eps", "weight_decay"] and sig.parameters["clip_value"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["lr"].default == 1e-3 and sig.parameters["betas"].default == (0.9, 0.999) and sig.parameters["clip_value"].default is None
    assert issubclass(cg.Adam, torch.optim.Adam) and cg.adam is adam and cg.AdamPlan is adam.AdamPlan
    mine, theirs = Toy(), Toy()
    a, b = cg.Adam(mine.parameters(), lr=5e-3, betas=(0.5, 0.9), weight_decay=0.01), torch.optim.Adam(theirs.parameters(), lr=5e-3, betas=(0.5, 0.9), weight_decay=0.01)
    _run(mine, a, 4), _run(theirs, b, 4)
    assert all(torch.equal(eref.bits(p), eref.bits(q)) for p, q in zip(mine.parameters(), theirs.parameters()))
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["state"].keys() == sb["state"].keys() == {0, 1} and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sa["state"].values())
    assert all(float(sa["state"][i]["step"]) == 4 and torch.equal(sa["state"][i]["exp_avg_sq"], sb["state"][i]["exp_avg_sq"]) for i in (0, 1))
    assert [set(g) - {"params"} for g in sa["param_groups"]] == [set(g) - {"params"} for g in sb["param_groups"]]
    assert a._groups[0].plan is None and len(a._groups[0].rest) == 3


def test_state_dicts_load_in_both_directions_mid_run():
    ref, x, y = Toy(), Toy(), Toy()
    o_ref = torch.optim.Adam(ref.parameters(), lr=5e-3, betas=(0.5, 0.9))
    _run(ref, o_ref, 6)
    o_x = torch.optim.Adam(x.parameters(), lr=5e-3, betas=(0.5, 0.9))
    _run(x, o_x, 2)
    o_y = cg.Adam(y.parameters(), lr=5e-3, betas=(0.5, 0.9))
    y.load_state_dict(x.state_dict())
    o_y.load_state_dict(o_x.state_dict())                        # torch -> cg
    _run(y, o_y, 2, start=2)
    o_x2 = torch.optim.Adam(x.parameters(), lr=5e-3, betas=(0.5, 0.9))
    x.load_state_dict(y.state_dict())
    o_x2.load_state_dict(o_y.state_dict())                       # cg -> torch
    _run(x, o_x2, 2, start=4)
    assert all(torch.equal(eref.bits(p), eref.bits(q)) for p, q in zip(x.parameters(), ref.parameters()))
    assert float(o_x2.state[x.a]["step"]) == 6


def test_the_clip_of_torchs_path_is_clamp_first():
    mine, theirs = Toy(), Toy()
    a, b = cg.Adam(mine.parameters(), lr=5e-3, clip_value=0.25), torch.optim.Adam(theirs.parameters(), lr=5e-3)
    for k in range(3):
        for model, opt in ((mine, a), (theirs, b)):
            opt.zero_grad(set_to_none=True)
            model.loss(k).backward()
        torch.nn.utils.clip_grad_value_(theirs.parameters(), 0.25)
        a.step(), b.step()
    assert all(torch.equal(eref.bits(p), eref.bits(q)) for p, q in zip(mine.parameters(), theirs.parameters()))
    assert float(mine.b.grad.abs().max()) == 0.25               # (the fallback's clip writes the gradient, as clip_grad_value_ does)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="Invalid clip_value"):
            cg.Adam(Toy().parameters(), clip_value=bad)


def test_attach_ema_refuses_what_it_cannot_take():
    m = Toy()
    opt = cg.Adam([m.a, m.b])
    with pytest.raises(TypeError, match="Adam.attach_ema: StandIn is not a control_gic_amd.LitEma"):
        opt.attach_ema(eref.StandIn(m), m)
    with pytest.raises(ValueError, match="Adam.attach_ema: this optimiser owns no parameter"):
        opt.attach_ema(cg.LitEma(eref.Small()), eref.Small())
    e = cg.LitEma(m)
    opt.attach_ema(e, m), opt.attach_ema(e, m)
    assert len(opt._attached) == 1 and e._fused_pending is None
    # on the CPU nothing rides: the step leaves the ema alone and ema(m) is the plain update
    before = e.a.clone()
    _run(m, opt, 1)
    assert e._fused_pending is None and torch.equal(e.a, before)
    e(m)
    assert torch.equal(eref.bits(e.a), eref.bits(eref.step(before, m.a.detach(), eref.one_minus_decay(0.9999))))


# ---------------------------------------------------------------------------- install()
def _model():
    model = Toy()
    model.quantize = cg.VectorQuantize2(64, 4, beta=0.25)
    model.encoder = eref.Small()
    return model


def test_install_leaves_configure_optimizers_alone_unless_asked():
    params = inspect.signature(cg.install).parameters
    assert params["patch_optimizers"].default is False and params["clip_value"].default is None
    model = _model()
    before = model.configure_optimizers
    cg.install(model)
    assert model.configure_optimizers == before and type(model.configure_optimizers()[0][0]) is torch.optim.Adam
    with pytest.raises(ValueError, match="install: clip_value is the clip of the cg.Adam that patch_optimizers=True swaps in"):
        cg.install(_model(), clip_value=1.0)


def test_install_patch_optimizers_swaps_exactly_torch_adam():
    model = _model()
    cg.install(model, patch_optimizers=True, clip_value=1.0)
    (first, second), schedulers = model.configure_optimizers()
    assert type(first) is cg.Adam and type(second) is torch.optim.SGD and schedulers == []
    assert first.clip_value == 1.0 and first.defaults["lr"] == 5e-5 and first.defaults["betas"] == (0.5, 0.9)
    assert [p is q for p, q in zip(first.param_groups[0]["params"], (model.a, model.b))] == [True, True] and first.param_groups[0]["lr"] == 5e-5
    _run(model, first, 2)
    ref = Toy()
    opt = torch.optim.Adam([ref.a, ref.b], lr=5e-5, betas=(0.5, 0.9))
    for k in range(2):
        opt.zero_grad(set_to_none=True)
        ref.loss(k).backward()
        torch.nn.utils.clip_grad_value_([ref.a, ref.b], 1.0)
        opt.step()
    assert torch.equal(eref.bits(model.a), eref.bits(ref.a)) and torch.equal(eref.bits(model.b), eref.bits(ref.b))


def test_install_attaches_the_models_emas_to_the_optimiser_that_owns_them():
    model = _model()
    model.ema_encoder = eref.StandIn(model.encoder)
    model.configure_optimizers = lambda: ([torch.optim.Adam(model.encoder.parameters(), lr=5e-5), torch.optim.Adam([model.a], lr=5e-5)], [])
    cg.install(model, patch_ema=True, patch_optimizers=True)
    (enc, other), _ = model.configure_optimizers()
    assert type(model.ema_encoder) is cg.LitEma and [e for e, _ in enc._attached] == [model.ema_encoder] and enc._attached[0][1] is model.encoder
    assert type(other) is cg.Adam and other._attached == [] and other.clip_value is None
