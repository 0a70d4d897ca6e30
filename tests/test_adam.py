"""The multi-tensor Adam on the GPU (csrc/cgic_adam.hip through control_gic_amd/adam.py) against tests/adam_ref.py run on the CPU.  Every
comparison with the restatement is on BITS of p, m, v, s and the step counts: the kernel states one fp32 rounding per operation, so
there is no tolerance (adam_ref.same_bits lets a NaN equal a NaN of another payload and nothing else).  Only the comparison of cg.Adam
with torch.optim.Adam has a bar: against the float64 chain, at most 4x torch's own error per tensor."""
import itertools

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import adam
import adam_ref as aref
import ema_ref as eref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CANARY = -12345.6789
GAP = 8
C = 4096
LR, BETAS = 5e-5, (0.5, 0.9)


class Carved:
    """tensors carved out of ONE device buffer with canary gaps between them: tensor i starts `offs[i]` elements behind a 16-byte
    boundary.  `cpu` are the host copies the restatement runs on"""

    def __init__(self, sizes, offs, seed, make=None):
        rng = np.random.default_rng(seed)
        starts, at = [], 4
        for n, o in zip(sizes, offs):
            starts.append(at + o)
            at = -(-(at + o + n + GAP) // 4) * 4
        host = np.full(at + 4, CANARY, np.float32)
        self.inside = np.zeros(at + 4, bool)
        self.spans = list(zip(starts, sizes))
        for a, n in self.spans:
            host[a:a + n] = (make or (lambda r, k: r.standard_normal(k)))(rng, n).astype(np.float32)
            self.inside[a:a + n] = True
        self.host = host
        self.dev = torch.from_numpy(host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.views = [self.dev[a:a + n] for a, n in self.spans]
        self.cpu = [host[a:a + n].copy() for a, n in self.spans]

    def gaps_unchanged(self):
        return bool((self.dev.cpu().numpy()[~self.inside] == np.float32(CANARY)).all())

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host.view(np.uint32))


def positive(rng, n):
    return np.abs(rng.standard_normal(n)) * 0.01


def wide(rng, n):
    """gradients spanning 1e-6 .. 1e2 in size"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)


def same(views, want):
    return all(aref.same_bits(v.cpu().numpy(), w) for v, w in zip(views, want) if w is not None)


def scalars(decay=0.9999, n=0):
    return torch.tensor(decay, dtype=torch.float32, device=DEV), (None if n is None else torch.tensor(n, dtype=torch.int32, device=DEV))


class Case:
    """the five carved operands of a list of sizes with the plan over them and the restatement's state beside it"""

    def __init__(self, sizes, po, so, go, seed, shadow=True, emas=None, ema_group=None, steps0=None, grad=wide):
        n = len(sizes)
        self.P, self.M = Carved(sizes, po, seed), Carved(sizes, so, seed + 1)
        self.V, self.G = Carved(sizes, so, seed + 2, positive), Carved(sizes, go, seed + 3, grad)
        self.S = Carved(sizes, [(a + b) % 4 for a, b in zip(po, so)], seed + 4) if shadow else None
        self.emas_host = [list(e) for e in (emas if emas is not None else ([(0.9999, 0)] if shadow else []))]
        self.emas_dev = [scalars(d, c) for d, c in self.emas_host]
        self.ema_group = ema_group
        self.steps_host = np.array(steps0 if steps0 is not None else [i % 5 for i in range(n)], np.float32)
        self.steps = torch.from_numpy(self.steps_host.copy()).to(DEV)
        shadows = self.S.views if shadow else None
        self.plan = cg.AdamPlan(self.P.views, self.M.views, self.V.views, self.steps, shadows, ema_group, self.emas_dev)
        self.p, self.m, self.v, self.s = self.P.cpu, self.M.cpu, self.V.cpu, (self.S.cpu if shadow else None)

    def step(self, present=None, lr=LR, lr_host=None, **kw):
        """one step on the device and in the restatement; present: which entries have a gradient (None: all)"""
        n = len(self.p)
        present = [True] * n if present is None else present
        self.plan.step([g if ok else None for g, ok in zip(self.G.views, present)], lr, BETAS, **kw)
        grads = [g if ok else None for g, ok in zip(self.G.cpu, present)]
        self.p, self.m, self.v, self.steps_host, self.s = aref.step(self.p, grads, self.m, self.v, self.steps_host, lr if lr_host is None else lr_host, BETAS,
                                                                     shadows=self.s, ema_group=self.ema_group, emas=self.emas_host, **kw)

    def check(self):
        assert same(self.P.views, self.p) and same(self.M.views, self.m) and same(self.V.views, self.v)
        assert np.array_equal(self.steps.cpu().numpy(), self.steps_host)
        assert self.P.gaps_unchanged() and self.M.gaps_unchanged() and self.V.gaps_unchanged() and self.G.unchanged()
        if self.S is not None:
            assert same(self.S.views, self.s) and self.S.gaps_unchanged()
        for (_, cnt), (_, want) in zip(self.emas_dev, self.emas_host):
            assert want is None or int(cnt) == want


# ---------------------------------------------------------------------------- sizes and geometry
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["no-decay", "decay"])
@pytest.mark.parametrize("clip", [None, 1.0], ids=["no-clip", "clip"])
@pytest.mark.parametrize("shadow", [False, True], ids=["no-shadow", "shadow"])
def test_every_size_at_every_offset_between_canaries(shadow, clip, wd):
    """0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 elements, each with param, gradient and state 0 to 3 elements behind a
    16-byte boundary in all 64 combinations: the 4-byte path runs next to the 16-byte one and nothing outside the tensors changes"""
    sizes, po, so, go = [], [], [], []
    for n in (0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1):
        for a, b, c in itertools.product(range(4), repeat=3):
            sizes.append(n), po.append(a), so.append(b), go.append(c)
    case = Case(sizes, po, so, go, 100, shadow=shadow)
    info = case.plan.info
    assert info["entries"] == 576 and info["chunk_elements"] == C and info["chunks"] == sum(-(-n // C) for n in sizes) == info["grid"] == 64 * 11
    want16 = sum(-(-n // C) for n, a, b in zip(sizes, po, so) if a == 0 and b == 0)
    assert info["chunks_16"] == want16 and 0 < want16 < info["chunks"] and info["shadowed"] == (576 if shadow else 0)
    for _ in range(2):
        case.step(eps=1e-8, weight_decay=wd, clip_value=clip)
    case.check()
    assert case.plan.info["uploads"] == 1 and case.plan.info["steps"] == 2


def test_700_small_tensors_and_one_of_40_chunks():
    sizes = [1 + i % 7 for i in range(700)] + [40 * C]
    case = Case(sizes, [i % 4 for i in range(701)], [(i // 4) % 4 for i in range(701)], [(i // 16) % 4 for i in range(701)], 200)
    assert case.plan.info["chunks"] == 740 and 0 < case.plan.info["chunks_16"] < 740
    case.step(clip_value=1.0)
    case.check()


def test_more_chunks_than_the_grid():
    """2050 chunks of one tensor on a grid of 2048: two workgroups take a second trip"""
    case = Case([2049 * C + 5, 3], [0, 1], [0, 2], [0, 3], 300)
    assert case.plan.info["chunks"] == 2051 and case.plan.info["grid"] == 2048
    case.step(clip_value=1.0, weight_decay=0.01)
    case.check()


# ---------------------------------------------------------------------------- absent gradients and the table of addresses
def test_absent_gradients_and_the_upload_of_their_table():
    """without a gradient: with a shadow the EMA alone, without one nothing, the step count stays; the table of gradient addresses
    goes up only when it changed"""
    sizes = [5, C + 3, 7, 64, 2 * C, 1]
    group = [0, 0, -1, -1, 0, -1]
    case = Case(sizes, [0, 1, 2, 3, 0, 1], [0] * 6, [1, 0, 0, 2, 0, 3], 400, ema_group=None)
    case.plan.close()
    # (shadows on entries 0, 1, 4 only)
    shadows = [v if g >= 0 else None for v, g in zip(case.S.views, group)]
    case.plan = cg.AdamPlan(case.P.views, case.M.views, case.V.views, case.steps, shadows, group, case.emas_dev)
    case.s, case.ema_group = [s if g >= 0 else None for s, g in zip(case.s, group)], group
    assert case.plan.info["shadowed"] == 3 and case.plan.info["uploads"] == 0
    before = [case.S.views[i].clone() for i in (2, 3, 5)]
    present = [True, False, True, False, False, True]
    case.step(present, clip_value=1.0)
    assert case.plan.info["uploads"] == 1
    case.step(present, clip_value=1.0)
    assert case.plan.info["uploads"] == 1 and case.plan.info["steps"] == 2            # the same table: nothing goes up
    assert list(case.steps_host) == [2, 1, 4, 3, 4, 2]
    case.step([False, True, True, True, False, False], clip_value=1.0)
    assert case.plan.info["uploads"] == 2
    case.step([False] * 6)
    case.step(None)
    assert case.plan.info["uploads"] == 4 and case.plan.info["upload_waits"] == 0
    case.S, spare = None, case.S
    case.check()
    assert same([spare.views[i] for i in (0, 1, 4)], [case.s[i] for i in (0, 1, 4)]) and spare.gaps_unchanged()
    assert all(torch.equal(spare.views[i], b) for i, b in zip((2, 3, 5), before))
    assert int(case.emas_dev[0][1]) == 5


# ---------------------------------------------------------------------------- special values
SPECIAL = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5e-39, 3.4e38, -3.4e38, 1.0, 1.0000001, -2.0], np.float32)


def special(rng, n):
    v = wide(rng, n).astype(np.float32)
    k = min(2 * len(SPECIAL), n // 3)
    v[rng.permutation(n)[:k]] = np.tile(SPECIAL, 2)[:k]
    return v


@pytest.mark.parametrize("n0", [-1, 0, (1 << 31) - 2])
@pytest.mark.parametrize("eps", [1e-8, 0.0])
def test_special_values_counters_and_two_ema_groups(eps, n0):
    """NaN, Inf and denormal gradients; exp_avg_sq of 0 with eps 0 (0 / 0 where the gradient is 0 too); two EMA groups with different
    counters in one plan, one of them at -1, 0 or 2^31 - 2"""
    sizes = [C + 37, 90, 29, 5]
    case = Case(sizes, [0, 1, 0, 2], [0, 0, 3, 1], [0, 2, 1, 0], 500, emas=[(0.9999, n0), (0.5, 41)], ema_group=[0, 1, 0, 1], grad=special)
    for t in (case.V, case.M):                               # exp_avg_sq and exp_avg of 0 on entry 2, where some gradients are 0
        t.views[2].zero_()
    case.v[2], case.m[2] = np.zeros(29, np.float32), np.zeros(29, np.float32)
    for clip in (None, 1.0):
        case.step(eps=eps, clip_value=clip)
    case.check()
    assert int(case.emas_dev[0][1]) == (n0 if n0 < 0 else eref._wrap32(n0 + 2)) and int(case.emas_dev[1][1]) == 43          # (2^31 - 2 wraps, like an int32 tensor)
    assert any(np.isnan(p).any() for p in case.p) and (eps != 0.0 or np.isnan(case.p[2]).any())


def test_a_nan_decay_stays_nan():
    case = Case([5, 9], [0, 1], [0, 0], [0, 0], 600, emas=[(float("nan"), 0)])
    case.step()
    case.check()
    assert all(np.isnan(s).all() for s in case.s) and int(case.emas_dev[0][1]) == 1


# ---------------------------------------------------------------------------- ordering and capture
def test_five_steps_eager_and_as_a_replayed_graph_with_a_device_lr():
    sizes = [3, C + 5, 64, 1]
    rng = np.random.default_rng(700)
    stage = [[wide(rng, n).astype(np.float32) for n in sizes] for _ in range(3)]
    stage_dev = [[torch.from_numpy(a).to(DEV) for a in row] for row in stage]
    lr = torch.tensor(LR, dtype=torch.float32, device=DEV)

    def fresh():
        return Case(sizes, [1, 0, 0, 2], [0, 0, 3, 2], [0, 0, 1, 0], 701, steps0=[0, 0, 0, 0])

    def load(case, row):
        for dst, src, host, values, (a, n) in zip(case.G.views, stage_dev[row], case.G.cpu, stage[row], case.G.spans):
            dst.copy_(src)
            host[:] = values
            case.G.host[a:a + n] = values

    eager = fresh()
    for k in range(5):                                           # nothing but stream order between them
        load(eager, k % 3)
        eager.step(lr=lr, lr_host=np.float32(LR if k <= 2 else 3e-4), clip_value=1.0)
        if k == 2:
            lr.fill_(3e-4)
    eager.check()
    assert eager.plan.info["uploads"] == 1
    lr.fill_(LR)
    # the same five as five replays of ONE captured step: gradients arrive in the fixed buffers, lr changes on the device
    graphed = fresh()
    load(graphed, 0)
    graphed.step(lr=lr, lr_host=np.float32(LR), clip_value=1.0)            # (eagerly first: the table of gradient addresses goes up here)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.plan.step(graphed.G.views, lr, BETAS, clip_value=1.0)
        # a changed table under capture is refused before anything is enqueued
        steps_before = graphed.plan.info["steps"]
        with pytest.raises(cg.CgicError, match="the gradient addresses changed while the stream is capturing") as got:
            graphed.plan.step([None] + graphed.G.views[1:], lr, BETAS, clip_value=1.0)
        assert got.value.code == cg._lib.ERR_INVALID and graphed.plan.info["steps"] == steps_before and graphed.plan.info["uploads"] == 1
    for k in range(1, 5):
        load(graphed, k % 3)
        g.replay()
        if k == 2:
            lr.fill_(3e-4)
    torch.cuda.synchronize()
    assert graphed.plan.info["uploads"] == 1
    for a, b in ((eager.P, graphed.P), (eager.M, graphed.M), (eager.V, graphed.V), (eager.S, graphed.S)):
        assert np.array_equal(a.dev.cpu().numpy().view(np.uint32), b.dev.cpu().numpy().view(np.uint32))
    assert torch.equal(eager.steps, graphed.steps) and int(graphed.emas_dev[0][1]) == 5 and float(graphed.steps[0]) == 5


# ---------------------------------------------------------------------------- the optimiser
class Mixed(torch.nn.Module):
    """fp32 parameters with one fp16 and one non-contiguous one among them, and one that never gets a gradient"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(60)
        self.a = torch.nn.Parameter(torch.randn(C + 33, generator=g))
        self.h = torch.nn.Parameter(torch.randn(17, generator=g).half())
        self.b = torch.nn.Parameter(torch.randn(4, 9, generator=g))
        self.t = torch.nn.Parameter(torch.randn(5, 3, generator=g).t())
        self.c = torch.nn.Parameter(torch.randn((), generator=g))
        self.idle = torch.nn.Parameter(torch.randn(6, generator=g))


NAMES = ("a", "h", "b", "t", "c")


@pytest.fixture(scope="module")
def gradient_rows():
    rng = np.random.default_rng(61)
    shapes = {k: tuple(p.shape) for k, p in Mixed().named_parameters()}
    rows = [{k: (wide(rng, int(np.prod(shapes[k], dtype=int))) * 0.01).astype(np.float32).reshape(shapes[k]) for k in NAMES} for _ in range(20)]
    for row in rows:                                            # the half parameter: sizes its type carries (1e-2 .. 1: no square underflows to 0)
        row["h"] = (rng.standard_normal(shapes["h"]) * 10.0 ** rng.uniform(-2, 0, shapes["h"])).astype(np.float32)
    return rows


def set_grads(m, row):
    for k in NAMES:
        p = getattr(m, k)
        p.grad = torch.from_numpy(row[k]).to(device=p.device, dtype=p.dtype)
    m.idle.grad = None


def test_cg_adam_against_torch_adam_and_float64_with_state_dicts_crossing(gradient_rows):
    """20 steps on a module mixing kernel-taken and fallback parameters, at step 10 each state_dict loaded into an optimiser of the
    other class: against the float64 chain every route's error is at most 4x that of torch.optim.Adam alone, per tensor"""
    kw = dict(lr=5e-3, betas=BETAS, weight_decay=0.01)
    models = {r: Mixed().to(DEV) for r in ("torch", "cg", "torch-then-cg", "cg-then-torch")}
    assert not models["cg"].t.is_contiguous() and models["cg"].h.dtype == torch.float16
    opts = {"torch": torch.optim.Adam(models["torch"].parameters(), **kw), "cg": cg.Adam(models["cg"].parameters(), **kw),
            "torch-then-cg": torch.optim.Adam(models["torch-then-cg"].parameters(), **kw), "cg-then-torch": cg.Adam(models["cg-then-torch"].parameters(), **kw)}
    exact = {k: [p.detach().cpu().double().numpy(), 0.0, 0.0] for k, p in Mixed().named_parameters() if k in NAMES}
    for t, row in enumerate(gradient_rows, 1):
        if t == 11:
            for r, cls in (("torch-then-cg", cg.Adam), ("cg-then-torch", torch.optim.Adam)):
                sd = opts[r].state_dict()
                assert all(s["step"].device.type == "cpu" and float(s["step"]) in (0, 10) for s in sd["state"].values())      # (0: the parameter that never has a gradient)
                opts[r] = cls(models[r].parameters(), **kw)
                opts[r].load_state_dict(sd)
        for r in models:
            set_grads(models[r], row)
            opts[r].step()
        for k in NAMES:
            g = torch.from_numpy(row[k]).to(models["cg"].state_dict()[k].dtype).double().numpy()
            exact[k] = list(aref.step64(exact[k][0], g, exact[k][1], exact[k][2], t, kw["lr"], BETAS, weight_decay=0.01))
    g = opts["cg"]._groups[0]
    assert [id(p) for p in g.taken] == [id(getattr(models["cg"], k)) for k in ("a", "b", "c", "idle")] and len(g.rest) == 2 and g.plan.info["entries"] == 4
    assert g.plan.info["uploads"] >= 1 and list(g.steps.cpu().numpy()) == [20, 20, 20, 0] and float(opts["cg"].state[models["cg"].a]["step"]) == 20
    assert opts["cg"].state[models["cg"].a]["step"].data_ptr() == g.steps.data_ptr()
    err = {r: {k: np.abs(getattr(models[r], k).detach().cpu().double().numpy() - exact[k][0]).max() for k in NAMES} for r in models}
    for r in ("cg", "torch-then-cg", "cg-then-torch"):
        for k in NAMES:
            print(f"{r} {k}: error {err[r][k]:.3e}, torch's {err['torch'][k]:.3e}")
            assert err["torch"][k] > 0 and err[r][k] <= 4 * err["torch"][k], (r, k, err[r][k], err["torch"][k])
    for k in ("h", "t"):                                        # torch's own path: the same bits
        assert torch.equal(getattr(models["cg"], k), getattr(models["torch"], k))
    assert torch.equal(models["cg"].idle, Mixed().idle.to(DEV))


def test_the_kernel_taken_parameters_are_adam_refs_bits(gradient_rows):
    m = Mixed().to(DEV)
    opt = cg.Adam(m.parameters(), lr=LR, betas=BETAS, clip_value=0.01)
    p = [getattr(Mixed(), k).detach().numpy().reshape(-1).copy() for k in ("a", "b", "c")]
    mm, vv, T = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p], np.zeros(3, np.float32)
    for row in gradient_rows[:3]:
        set_grads(m, row)
        raw = m.a.grad.clone()
        opt.step()
        assert torch.equal(m.a.grad, raw)                       # the fused clip does not write the gradient
        assert float(m.h.grad.abs().max()) <= 0.0101            # ... the fallback's does (0.01 in fp16 is 0.010002)
        p, mm, vv, T, _ = aref.step(p, [row[k].reshape(-1) for k in ("a", "b", "c")], mm, vv, T, LR, BETAS, clip_value=0.01)
    for k, want, wm in zip(("a", "b", "c"), p, mm):
        assert aref.same_bits(getattr(m, k).detach().cpu().numpy().reshape(-1), want)
        assert aref.same_bits(opt.state[getattr(m, k)]["exp_avg"].cpu().numpy().reshape(-1), wm)


def test_step_issues_no_synchronising_call(gradient_rows):
    m = Mixed().to(DEV)
    opt = cg.Adam(m.parameters(), lr=LR, betas=BETAS, clip_value=1.0)
    e = cg.LitEma(m, 0.9999, use_num_upates=True).to(DEV)
    opt.attach_ema(e, m)
    set_grads(m, gradient_rows[0])
    opt.step(), e(m)                                            # (the plan is built here: an upload)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for row in gradient_rows[1:3]:
            for k in ("a", "b", "c"):                           # (new gradient tensors every step, as after zero_grad: made without a host copy)
                getattr(m, k).grad = getattr(m, k).grad * 0.5
            opt.step(), e(m)
        with pytest.raises(RuntimeError):                       # (the mode does see a read on the host)
            float(opt.state[m.a]["step"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(opt.state[m.a]["step"]) == 3 and int(e.num_updates) == 3 and 1 <= opt._groups[0].plan.info["uploads"] <= 3


def test_attached_ema_equals_the_step_followed_by_litema(gradient_rows):
    """parameters and shadows after opt.step(); ema(module) with the ema attached equal those of cg.Adam followed by cg.LitEma, bit for
    bit, pairs on torch's path included; num_updates moves once per step; a forward without a fused step before it is the plain one"""
    ma, mb = Mixed().to(DEV), Mixed().to(DEV)
    oa, ob = cg.Adam(ma.parameters(), lr=5e-3, betas=BETAS, clip_value=1.0), cg.Adam(mb.parameters(), lr=5e-3, betas=BETAS, clip_value=1.0)
    ea, eb = cg.LitEma(ma, 0.9999, use_num_upates=True).to(DEV), cg.LitEma(mb, 0.9999, use_num_upates=True).to(DEV)
    oa.attach_ema(ea, ma)
    for step, row in enumerate(gradient_rows[:5], 1):
        for m, o, e in ((ma, oa, ea), (mb, ob, eb)):
            set_grads(m, row)
            o.step()
            if m is ma:
                assert int(e.num_updates) == step and e._fused_pending is not None
            e(m)
        assert int(ea.num_updates) == int(eb.num_updates) == step and ea._fused_pending is None
        for k, sname in ea.m_name2s_name.items():
            assert torch.equal(eref.bits(dict(ma.named_parameters())[k]), eref.bits(dict(mb.named_parameters())[k])), (step, k)
            assert torch.equal(eref.bits(ea._buffers[sname]), eref.bits(eb._buffers[sname])), (step, k)
    g = oa._groups[0]
    assert g.plan.info["shadowed"] == 4 and g.plan.info["ema_groups"] == 1 and len(g.owned[id(ea)]) == 4 and ea._plan is None
    ea(ma), eb(mb)                                              # no fused step before it: the plain update, counter included
    assert int(ea.num_updates) == int(eb.num_updates) == 6
    assert all(torch.equal(eref.bits(ea._buffers[s]), eref.bits(eb._buffers[s])) for s in ea.m_name2s_name.values())


def test_the_op_equals_the_class(gradient_rows):
    m = Mixed().to(DEV)
    opt = cg.Adam([m.a, m.b, m.c], lr=LR, betas=BETAS, weight_decay=0.01, clip_value=1.0)
    e = cg.LitEma(m, 0.9999, use_num_upates=True).to(DEV)
    names = ("a", "b", "c")
    params = [getattr(m, k).detach().clone() for k in names]
    ms, vs = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    shadows = [e._buffers[k].clone() for k in names]
    steps, (decay, n) = torch.zeros(3, device=DEV), scalars(0.9999, 0)
    sub = torch.nn.Module()
    for k in names:
        sub.register_parameter(k, getattr(m, k))
    e2 = cg.LitEma(sub, 0.9999, use_num_upates=True).to(DEV)
    opt.attach_ema(e2, sub)
    for row in gradient_rows[:2]:
        set_grads(m, row)
        opt.step()
        assert torch.ops.cgic.adam_step(params, [getattr(m, k).grad for k in names], ms, vs, steps, LR, BETAS[0], BETAS[1], 1e-8, 0.01, 1.0, None,
                                        shadows, decay, n) is None
    assert int(n) == int(e2.num_updates) == 2 and list(steps.cpu().numpy()) == [2, 2, 2]
    for k, p, mm, s in zip(names, params, ms, shadows):
        assert torch.equal(eref.bits(p), eref.bits(getattr(m, k))) and torch.equal(eref.bits(mm), eref.bits(opt.state[getattr(m, k)]["exp_avg"]))
        assert torch.equal(eref.bits(s), eref.bits(e2._buffers[k]))
    assert len(adam._plans) <= adam._PLAN_CACHE_SIZE
