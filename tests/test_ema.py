"""The multi-tensor EMA on the GPU (csrc/cgic_ema.hip through control_gic_amd/ema.py) against tests/ema_ref.py, the torch restatement
of the reference's LitEma, run on the CPU.  Every comparison is on BITS: the kernel states the reference's three fp32 roundings, so
there is no tolerance.  (ema_ref.same_bits lets a NaN equal a NaN of another payload -- which NaN an operation makes is outside
IEEE 754's contract -- and nothing else.)  Sizes come from cgic_ema_plan_info, so they follow the chunk the library was built with."""
import os

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import ema
import ema_ref as eref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ema.npz"))
RUNS = {"plain": False, "counted": True, "cross": True}
STEPS = 5
CANARY = -12345.6789
GAP = 8                     # elements between two tensors of a carved buffer, before the next 16-byte boundary


def chunk_elements():
    t = torch.zeros(4, device=DEV)
    return cg.EmaPlan([t], [t.clone()]).info["chunk_elements"]


class Carved:
    """tensors carved out of ONE buffer per side with canary gaps between them: tensor i starts `offs[i]` elements behind a 16-byte
    boundary.  The host copies are what the restatement runs on."""

    def __init__(self, sizes, offs, seed, shapes=None):
        rng = np.random.default_rng(seed)
        starts, at = [], 4
        for n, o in zip(sizes, offs):
            starts.append(at + o)
            at = -(-(at + o + n + GAP) // 4) * 4
        self.host = torch.full((at + 4,), CANARY, dtype=torch.float32)
        self.inside = torch.zeros(at + 4, dtype=torch.bool)
        self.spans = list(zip(starts, sizes))
        for a, n in self.spans:
            self.host[a:a + n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
            self.inside[a:a + n] = True
        self.dev = self.host.to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        shapes = shapes or [(n,) for n in sizes]
        self.views = [self.dev[a:a + n].view(s) for (a, n), s in zip(self.spans, shapes)]
        self.cpu = [self.host[a:a + n].clone().view(s) for (a, n), s in zip(self.spans, shapes)]

    def gaps_unchanged(self):
        got = self.dev.cpu()
        return bool((got[~self.inside] == CANARY).all())

    def unchanged(self):
        return torch.equal(eref.bits(self.dev), eref.bits(self.host))


def scalars(decay=0.9999, n=None):
    return torch.tensor(decay, dtype=torch.float32, device=DEV), (None if n is None else torch.tensor(n, dtype=torch.int32, device=DEV))


def all_same(gpu, cpu):
    return all(eref.same_bits(g, c) for g, c in zip(gpu, cpu))


# ---------------------------------------------------------------------------- sizes and geometry
OFFSETS = {"aligned": ((0,), (0,)), "shadows-off": ((1, 2, 3, 0), (0,)), "params-off": ((0,), (3, 0, 1, 2)), "both-off": ((1, 2, 3, 0), (2, 0, 3, 0))}


@pytest.mark.parametrize("which", OFFSETS)
def test_every_size_at_every_offset_between_canaries(which):
    """1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 chunk + 3, an empty tensor and a 0-dim one, each side as views 0 to 3 elements behind
    a 16-byte boundary: the 4-byte path runs next to the 16-byte one, and not an element outside the tensors changes"""
    c = chunk_elements()
    sizes = [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 3, 0, 1, 7, 2 * c]
    shapes = [(n,) for n in sizes]
    shapes[9] = ()                                               # the 0-dim parameter
    so, po = OFFSETS[which]
    S = Carved(sizes, [so[i % len(so)] for i in range(len(sizes))], 1, shapes)
    P = Carved(sizes, [po[i % len(po)] for i in range(len(sizes))], 2, shapes)
    plan = cg.EmaPlan(S.views, P.views)
    info = plan.info
    assert info["entries"] == len(sizes) and info["elements"] == sum(sizes) and info["chunks"] == sum(-(-n // c) for n in sizes) == info["grid"]
    want16 = sum(-(-n // c) for (a, n), (b, _) in zip(S.spans, P.spans) if a % 4 == 0 and b % 4 == 0)
    assert info["chunks_16"] == want16 and (0 < want16 < info["chunks"] if which != "aligned" else want16 == info["chunks"])
    decay, n = scalars(0.9, 3)
    plan.update(decay, n)
    want, n_after = eref.update(S.cpu, P.cpu, 0.9, 3)
    assert all_same(S.views, want) and int(n) == n_after == 4
    assert S.gaps_unchanged() and P.unchanged()


def test_700_small_tensors_and_one_of_40_chunks():
    c = chunk_elements()
    sizes = [1 + i % 7 for i in range(700)] + [40 * c]
    S, P = Carved(sizes, [i % 4 for i in range(701)], 3), Carved(sizes, [(i // 4) % 4 for i in range(701)], 4)
    plan = cg.EmaPlan(S.views, P.views)
    assert plan.info["chunks"] == 740 and 0 < plan.info["chunks_16"] < 740
    decay, _ = scalars(0.75)
    plan.update(decay)
    want, _ = eref.update(S.cpu, P.cpu, 0.75)
    assert all_same(S.views, want) and S.gaps_unchanged() and P.unchanged()


def test_more_chunks_than_the_grid_and_the_counter_moves_once():
    """3 200 chunks on a grid of 2 048: the small tensors are reached in the workgroups' second trip; every workgroup reads omd,
    one thread of another launch moved the counter"""
    c = chunk_elements()
    sizes = [2500 * c + 3] + [1 + i % 7 for i in range(699)]
    S, P = Carved(sizes, [0] + [i % 4 for i in range(699)], 5), Carved(sizes, [0] * 700, 6)
    plan = cg.EmaPlan(S.views, P.views)
    assert plan.info["chunks"] == 3200 and plan.info["grid"] == 2048 < plan.info["chunks"]
    decay, n = scalars(0.9999, 41)
    plan.update(decay, n)
    want, n_after = eref.update(S.cpu, P.cpu, 0.9999, 41)
    assert int(n) == n_after == 42
    assert all_same(S.views, want) and S.gaps_unchanged() and P.unchanged()


# ---------------------------------------------------------------------------- counter and decay
SPECIAL = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5e-39, 3.4e38, -3.4e38, 1.0], np.float32)


def _specials(n, seed):
    """random values with Inf, NaN, the zeros, denormals and the largest values sprinkled in (a quarter of a small tensor)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n).astype(np.float32)
    k = min(4 * len(SPECIAL), n // 4)
    v[rng.permutation(n)[:k]] = np.tile(SPECIAL, 4)[:k]
    return torch.from_numpy(v)


@pytest.fixture(scope="module")
def special_case():
    c = chunk_elements()
    sizes = [c + 37, 29, 5]
    shadows = [_specials(n, 10 + i) for i, n in enumerate(sizes)]
    params = [_specials(n, 20 + i) for i, n in enumerate(sizes)]
    shadows[1][:12], params[1][:12] = torch.from_numpy(SPECIAL), torch.ones(12)        # every special shadow against a finite parameter
    shadows[1][12:24], params[1][12:24] = torch.ones(12), torch.from_numpy(SPECIAL)    # ... and the other way round
    return shadows, params


@pytest.mark.parametrize("n0", [None, -1, 0, 89990, 89991, (1 << 24) + 1, (1 << 31) - 2])
@pytest.mark.parametrize("decay", [0.9999, 0.0, 1.0, 0.5])
def test_counter_decay_and_special_values(special_case, decay, n0):
    """num_updates of -1 stays and the plain decay is used; 0 becomes 1 and the decay is 2 / 11; either side of the crossing with
    0.9999; parameters and shadows holding Inf, NaN, -0.0 and denormals: NaN exactly where the restatement has NaN, every other bit equal"""
    shadows, params = special_case
    s, p = [t.to(DEV) for t in shadows], [t.to(DEV) for t in params]
    d, n = scalars(decay, n0)
    cg.EmaPlan(s, p).update(d, n)
    want, n_after = eref.update(shadows, params, decay, n0)
    assert n0 is None or int(n) == n_after == (n0 if n0 < 0 else n0 + 1)
    assert all_same(s, want)
    assert all(torch.equal(eref.bits(a), eref.bits(b)) for a, b in zip(p, params))
    if n0 == 0 and decay == 0.9999:
        assert eref.one_minus_decay(decay, n0) == np.float32(1.0) - np.float32(2.0) / np.float32(11.0)
    if eref.one_minus_decay(decay, n0) == 0:                   # (decay 1 without a counter, at -1, and where (1 + n) / (10 + n) is 1.0)
        # omd is 0: s - 0 * (s - p) keeps the bits of s wherever s - p is finite -- except a shadow of -0.0, which s - (-0.0) turns into
        # +0.0 when s - p is negative: the restatement says the same
        for a, b, q in zip(s, shadows, params):
            keep = torch.isfinite(b) & torch.isfinite(q) & torch.isfinite(b - q) & ~((b == 0) & torch.signbit(b))
            assert int(keep.sum()) > 0 and torch.equal(eref.bits(a)[keep], eref.bits(b)[keep])


def test_a_nan_decay_stays_nan():
    s, p = [torch.ones(5, device=DEV)], [torch.zeros(5, device=DEV)]
    d, n = scalars(float("nan"), 0)
    cg.EmaPlan(s, p).update(d, n)
    assert bool(torch.isnan(s[0]).all()) and int(n) == 1


# ---------------------------------------------------------------------------- ordering and capture
def test_five_updates_back_to_back_and_as_a_graph():
    c = chunk_elements()
    sizes = [3, c + 5, 64, 1]
    S, P = Carved(sizes, [1, 0, 0, 2], 40), Carved(sizes, [0, 0, 3, 2], 41)
    rng = np.random.default_rng(42)
    stage = [[torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in sizes] for _ in range(STEPS + 1)]
    stage_dev = [[t.to(DEV) for t in row] for row in stage]
    plan = cg.EmaPlan(S.views, P.views)
    decay, n = scalars(0.9999, 0)
    torch.cuda.synchronize()
    for k in range(STEPS):                                      # nothing but stream order between them
        for dst, src in zip(P.views, stage_dev[k]):
            dst.copy_(src)
        plan.update(decay, n)
    want, cnt = S.cpu, 0
    for k in range(STEPS):
        want, cnt = eref.update(want, stage[k], 0.9999, cnt)
    assert all_same(S.views, want) and int(n) == cnt == STEPS
    # the same five as one captured graph -- a linear chain of ten launches --, replayed on new parameter values in the same tensors
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.update(decay, n)                                   # (warm-up on the capture's side of things: one more step)
    torch.cuda.current_stream().wait_stream(side)
    want, cnt = eref.update(want, stage[STEPS - 1], 0.9999, cnt)
    with torch.cuda.graph(g):
        for k in range(STEPS):
            plan.update(decay, n)
    for row_dev, row in ((stage_dev[STEPS], stage[STEPS]), (stage_dev[0], stage[0])):
        for dst, src in zip(P.views, row_dev):
            dst.copy_(src)
        g.replay()
        for k in range(STEPS):
            want, cnt = eref.update(want, row, 0.9999, cnt)
        assert all_same(S.views, want) and int(n) == cnt
    assert cnt == 3 * STEPS + 1 and S.gaps_unchanged()


# ---------------------------------------------------------------------------- copies
def test_copy_to_store_and_restore_are_exact():
    c = chunk_elements()
    sizes = [1, 3, 4, 5, c - 1, c + 1, 2 * c + 3, 0, 6]
    S, P = Carved(sizes, [i % 4 for i in range(9)], 50), Carved(sizes, [(i // 2) % 4 for i in range(9)], 51)
    S.dev[S.inside.to(DEV)] = _specials(int(S.inside.sum()), 52).to(DEV)          # copies are bit for bit: NaN payloads and -0.0 included
    shadow_bits = [eref.bits(v).clone() for v in S.views]
    param_bits = [eref.bits(v).clone() for v in P.views]
    plan = cg.EmaPlan(S.views, P.views)
    assert 0 < plan.info["chunks_16_stash"] < plan.info["chunks"] and plan.info["stash_elements"] == sum(-(-n // 4) * 4 for n in sizes)
    stash = plan.new_stash()
    stash.fill_(CANARY)
    plan.copy("store", stash)
    kept = plan.stash_views(stash, [(n,) for n in sizes])
    assert all(torch.equal(eref.bits(k), b) for k, b in zip(kept, param_bits))
    used = torch.zeros(stash.numel(), dtype=torch.bool)
    at = 0
    for n in sizes:
        used[at:at + n] = True
        at += -(-n // 4) * 4
    assert bool((stash.cpu()[~used] == CANARY).all())
    plan.copy("copy_to")
    assert all(torch.equal(eref.bits(v), b) for v, b in zip(P.views, shadow_bits)) and P.gaps_unchanged()
    plan.copy("restore", stash)
    assert all(torch.equal(eref.bits(v), b) for v, b in zip(P.views, param_bits)) and P.gaps_unchanged()
    assert all(torch.equal(eref.bits(v), b) for v, b in zip(S.views, shadow_bits)) and S.gaps_unchanged()
    with pytest.raises(ValueError, match="EmaPlan.copy: stash torch.float32 of 3 elements"):
        plan.copy("store", torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="EmaPlan.copy: direction 'sideways'"):
        plan.copy("sideways")


def test_store_is_one_allocation():
    m = eref.Small().load(GOLDEN, "plain/init").to(DEV)
    e = cg.LitEma(m)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
    e.store(m.parameters())
    assert torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before == 1
    params = list(m.parameters())
    assert len(e.collected_params) == len(params) and all(torch.equal(eref.bits(c), eref.bits(p)) for c, p in zip(e.collected_params, params))
    base = e.collected_params[0].untyped_storage().data_ptr()
    assert all(c.untyped_storage().data_ptr() == base for c in e.collected_params)
    # the plan of the parameter list is the module's own (not the op's cache) and is kept for the next store
    mine, cached = e._store_plan, len(ema._plans)
    e.store(m.parameters())
    assert e._store_plan is mine and len(ema._plans) == cached


# ---------------------------------------------------------------------------- the module and the op
def _run_module(make, tag):
    m = eref.Small().load(GOLDEN, tag + "/init").to(DEV)
    e = make(m, RUNS[tag]).to(DEV)
    e.num_updates.fill_(int(GOLDEN[tag + "/start"]))
    frozen = m.frozen.detach().clone()
    for step in range(STEPS):
        m.load(GOLDEN, f"{tag}/param{step}")
        frozen = m.frozen.detach().clone()
        e(m)
        assert int(e.num_updates) == int(GOLDEN[f"{tag}/num_updates{step}"])
        for k, sname in e.m_name2s_name.items():
            assert torch.equal(eref.bits(e._buffers[sname]), eref.bits(torch.from_numpy(GOLDEN[f"{tag}/shadow{step}/{k}"]))), (tag, step, k)
        assert torch.equal(m.frozen, frozen)
    assert e._plan is not None and e._plan.info["entries"] == len(e.m_name2s_name) == 6
    return m, e


@pytest.mark.parametrize("tag", RUNS)
def test_litema_reproduces_the_real_class_at_every_step(tag):
    m, e = _run_module(lambda m, counted: cg.LitEma(m, 0.9999, use_num_upates=counted), tag)
    # store / copy_to / restore on the module, as validation uses them (model.py: ema_scope)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    e.store(m.parameters())
    e.copy_to(m)
    assert all(torch.equal(eref.bits(p), eref.bits(e._buffers[e.m_name2s_name[k]])) for k, p in m.named_parameters() if p.requires_grad)
    assert torch.equal(m.frozen, before["frozen"])
    e.restore(m.parameters())
    assert all(torch.equal(eref.bits(p), eref.bits(before[k])) for k, p in m.named_parameters())


@pytest.mark.parametrize("tag", RUNS)
def test_an_adopted_litema_does_the_same(tag):
    _run_module(lambda m, counted: cg.LitEma.adopt(eref.StandIn(m, 0.9999, use_num_upates=counted)), tag)


def test_the_plan_follows_the_tensors_when_they_move():
    m = eref.Small().load(GOLDEN, "plain/init").to(DEV)
    e = cg.LitEma(m).to(DEV)
    e(m)
    first = e._plan
    e(m)
    assert e._plan is first
    with torch.no_grad():
        m.head.weight.data = m.head.weight.data.clone()         # one tensor somewhere else: what .to() does to all of them
    shadows = [e._buffers[e.m_name2s_name[k]].cpu() for k, p in m.named_parameters() if p.requires_grad]
    params = [p.detach().cpu() for p in m.parameters() if p.requires_grad]
    e(m)
    assert e._plan is not first
    want, _ = eref.update(shadows, params, 0.9999)
    assert all_same([e._buffers[e.m_name2s_name[k]] for k, p in m.named_parameters() if p.requires_grad], want)


class Mixed(torch.nn.Module):
    """fp32 parameters with one fp16 and one non-contiguous one among them"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(60)
        self.a = torch.nn.Parameter(torch.randn(33, generator=g))
        self.h = torch.nn.Parameter(torch.randn(17, generator=g).half())
        self.b = torch.nn.Parameter(torch.randn(4, 9, generator=g))
        self.t = torch.nn.Parameter(torch.randn(5, 3, generator=g).t())
        self.c = torch.nn.Parameter(torch.randn((), generator=g))


@pytest.mark.parametrize("counted", [False, True])
def test_pairs_the_kernel_does_not_take_get_torchs_expression(counted):
    m = Mixed()
    host = {k: p.detach().clone() for k, p in m.named_parameters()}
    m = m.to(DEV)
    assert not m.t.is_contiguous() and m.h.dtype == torch.float16
    e = cg.LitEma(m, 0.9, use_num_upates=counted).to(DEV)
    shadows = {k: v.clone() for k, v in host.items()}
    cnt = 0 if counted else None
    rng = np.random.default_rng(61)
    for step in range(3):
        with torch.no_grad():
            for k, p in m.named_parameters():
                host[k] = host[k] + torch.from_numpy(rng.standard_normal(tuple(host[k].shape)).astype(np.float32)).to(host[k].dtype)
                p.copy_(host[k])
        e(m)
        new, cnt = eref.update([shadows[k] for k in host], [host[k] for k in host], 0.9, cnt)
        shadows = dict(zip(host, new))
        for k in host:
            assert eref.same_bits(e._buffers[k], shadows[k]), (step, k)
    assert e._plan.info["entries"] == 3 and int(e.num_updates) == (3 if counted else -1)


def test_the_op_equals_the_class():
    m = eref.Small().load(GOLDEN, "counted/init").to(DEV)
    e = cg.LitEma(m, 0.9999, use_num_upates=True).to(DEV)
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    shadows = [e._buffers[e.m_name2s_name[k]].clone() for k in names]
    params = [dict(m.named_parameters())[k].detach() for k in names]
    decay, n = e.decay.clone(), e.num_updates.clone()
    for step in range(2):
        m.load(GOLDEN, f"counted/param{step}")
        e(m)
        assert torch.ops.cgic.ema_update(shadows, params, decay, n) is None
        assert int(n) == int(e.num_updates) == step + 1
        assert all(torch.equal(eref.bits(a), eref.bits(e._buffers[e.m_name2s_name[k]])) for a, k in zip(shadows, names))
    torch.ops.cgic.ema_update([], [], decay, n)                 # no pair: the counter still moves
    assert int(n) == 3
    assert len(ema._plans) <= ema._PLAN_CACHE_SIZE


# ---------------------------------------------------------------------------- no host synchronisation
@pytest.mark.parametrize("module", ["small", "mixed"])
def test_forward_issues_no_synchronising_call(module):
    m = (eref.Small().load(GOLDEN, "counted/init") if module == "small" else Mixed()).to(DEV)
    e = cg.LitEma(m, 0.9999, use_num_upates=True).to(DEV)
    e(m)                                                        # (the plan is built here: an upload)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        e(m)
        e(m)
        with pytest.raises(RuntimeError):                       # (the mode does see a read on the host: the reference's `>= 0`)
            bool(e.num_updates >= 0)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert int(e.num_updates) == 3
