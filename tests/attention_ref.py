"""What the attention tests measure against (AttnBlock.forward: CGIC/modules/vqvae/decoder.py:189-213, vqvae_blocks.py:168-193),
on whichever device the inputs are:

  restatement(q, k, v)   the expression written out in float64 from the exactly upcast inputs -- the reference of the GPU tests;
                         tests/test_attention_host.py holds it (in fp32) to tests/golden/attn.npz, which the real class produced;
  torch_expr(q, k, v)    the same expression by torch's own ops in the operand type, as the model runs it today: for fp16 / bf16 the
                         chain autocast makes of it -- bmm in the half type, the scale in the half type, softmax in fp32, the
                         weights cast to the half type, bmm in the half type.  Its max-abs error against the float64 value is E_ref,
                         the unit of the tests' bars;
  lse64 / lse_torch32    ln sum_j exp(scale * s_ij) in float64, and by torch's fp32 logsumexp of fp32 scores;
  StandIn                a module with the reference's members and forward, for the module and install() tests.

Infinite and saturated scores (tests/test_attention_scores.py on the GPU, tests/test_attention_host.py on the CPU):
  SCORE_CASES / build_case  a seeded catalogue of edge cases, each with its expected NaN / +Inf / -Inf pattern spelled out by index;
  patterns / same_patterns  the three non-finite patterns of a tensor, which max_err does not compare;
  model_expr / e_model      the kernel's own precision model in torch ops (fp32 scores from the exactly upcast inputs, fp32 softmax,
                            weights rounded once to the operand type, fp32 second product) and its error E_model against float64:
                            the unit that stays meaningful where torch's half chain rounds scores of thousands to the half type;
  tiled_model               the kernel's tile loop in fp32 torch ops, with and without the guard of a leading all -inf tile;
  case_refs / judge         the references of a built case, and every assertion on a result (shared by the CPU and the GPU tests).
"""
import numpy as np
import torch

BAR_F32 = 4.0      # fp32: both sides are the same chain of roundings in another order (the project's SpatialNorm margin)
BAR_HALF = 1.0     # half inputs, fp32 out: the kernel keeps the scores in fp32 where torch rounds them: not worse than what it replaces
BAR_LSE = 4.0      # x torch's own fp32 logsumexp error


def _scale(c, scale):
    return int(c) ** (-0.5) if scale is None else scale


def restatement(q, k, v, scale=None, dtype=torch.float64):
    """[B,C,N] in `dtype` (float64) from the exactly upcast inputs"""
    q, k, v = (t.detach().to(dtype) for t in (q, k, v))
    b, c = q.shape[:2]
    q, k, v = (t.reshape(b, c, -1) for t in (q, k, v))
    w = torch.bmm(q.permute(0, 2, 1), k) * _scale(c, scale)
    w = torch.softmax(w, dim=2)
    return torch.bmm(v, w.permute(0, 2, 1))


def torch_expr(q, k, v, scale=None):
    """the reference's expression in the operand type (fp32: as written; halves: as under torch.autocast) -> [B,C,N] of that type"""
    b, c = q.shape[:2]
    q, k, v = (t.detach().reshape(b, c, -1) for t in (q, k, v))
    w = torch.bmm(q.permute(0, 2, 1), k)
    w = w * _scale(c, scale)
    w = torch.softmax(w.float(), dim=2).to(q.dtype)
    return torch.bmm(v, w.permute(0, 2, 1))


def lse64(q, k, scale=None):
    b, c = q.shape[:2]
    q, k = (t.detach().double().reshape(b, c, -1) for t in (q, k))
    return torch.logsumexp(torch.bmm(q.permute(0, 2, 1), k) * _scale(c, scale), dim=2)


def lse_torch32(q, k, scale=None):
    b, c = q.shape[:2]
    q, k = (t.detach().float().reshape(b, c, -1) for t in (q, k))
    return torch.logsumexp(torch.bmm(q.permute(0, 2, 1), k) * _scale(c, scale), dim=2)


def max_err(got, ref64):
    """(max-abs error over the finite elements of the reference, NaN patterns equal)"""
    got = got.detach().double().reshape(ref64.shape)
    ok = torch.isfinite(ref64)
    same_nan = bool(torch.equal(torch.isnan(got), torch.isnan(ref64)))
    return (float((got - ref64)[ok].abs().max()) if bool(ok.any()) else 0.0), same_nan


def e_ref(ref64, q, k, v, scale=None):
    """max-abs error of torch's own evaluation in the operand type against the float64 value"""
    return max_err(torch_expr(q, k, v, scale), ref64)[0]


def make_inputs(seed, B, C, N, dtype=torch.float32, gain=1.0):
    """q, k, v [B,C,N]: N(0,1), q times `gain`, rounded to `dtype`; seeded, on the CPU"""
    rng = np.random.default_rng(seed)
    t = lambda: torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32))
    q, k, v = t(), t(), t()
    return (q * gain).to(dtype), k.to(dtype), v.to(dtype)


class StandIn(torch.nn.Module):
    """the members and the forward of the reference's two AttnBlocks, for tests of the module swap (not the package's class):
    StandIn(C) the encoder's (a GroupNorm, forward(x)); StandIn(C, norm=module) the decoder's (forward(x, zq) hands zq to `norm`)"""

    def __init__(self, in_channels, norm=None):
        super().__init__()
        self.in_channels = in_channels
        self.takes_zq = norm is not None
        self.norm = norm if norm is not None else torch.nn.GroupNorm(num_groups=32, num_channels=in_channels, eps=1e-6, affine=True)
        for name in ("q", "k", "v", "proj_out"):
            setattr(self, name, torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0))

    def forward(self, x, zq=None):
        h_ = self.norm(x, zq) if self.takes_zq else self.norm(x)
        q, k, v = self.q(h_), self.k(h_), self.v(h_)
        b, c, h, w = q.shape
        q = q.reshape(b, c, h * w).permute(0, 2, 1)
        k = k.reshape(b, c, h * w)
        w_ = torch.bmm(q, k)
        w_ = w_ * (int(c) ** (-0.5))
        w_ = torch.nn.functional.softmax(w_, dim=2)
        v = v.reshape(b, c, h * w)
        h_ = torch.bmm(v, w_.permute(0, 2, 1)).reshape(b, c, h, w)
        return x + self.proj_out(h_)


def randomize(module, seed, noise=0.03):
    """parameters away from their initial values (a 1x1 conv of 256 channels starts within 1/16), seeded"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p + noise * torch.randn(p.shape, generator=g).to(p))
    return module


# ---------------------------------------------------------------------------------------------------------------------------------
# infinite and saturated scores
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_BK = 128      # kAttnBK (csrc/cgic_attn_plan.h): the keys of one tile of the kernel's online softmax
NEGLIGIBLE = -64.0 # kNegligible (csrc/cgic_attn.hip): the binary exponent below which a weight or a rescale factor is an exact 0
C0 = 7             # the channel of the plantings in q and k
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
INF = float("inf")


def patterns(t):
    """(NaN, +Inf, -Inf) masks of `t`"""
    t = t.detach()
    return torch.isnan(t), t == INF, t == -INF


def same_patterns(got, want):
    """the NaN, the +Inf and the -Inf pattern of `got` each equal those of `want` (a tensor, or a tuple of three masks)"""
    want = want if isinstance(want, tuple) else patterns(want)
    return all(bool(torch.equal(a, b.reshape(a.shape).to(a.device))) for a, b in zip(patterns(got), want))


def same_bits(a, b):
    """torch.equal that lets a NaN equal a NaN: the same NaN pattern and the same values everywhere else"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.masked_fill(na, 0), b.masked_fill(nb, 0)))


def model_expr(q, k, v, scale=None):
    """the kernel's precision model in torch ops: fp32 scores from the exactly upcast inputs, fp32 softmax, the weights rounded once
    to the operand type, fp32 second product -> fp32 [B,C,N].  For fp32 inputs this is torch_expr."""
    b, c = q.shape[:2]
    dt = q.dtype
    q, k, v = (t.detach().float().reshape(b, c, -1) for t in (q, k, v))
    w = torch.bmm(q.permute(0, 2, 1), k) * _scale(c, scale)
    w = torch.softmax(w, dim=2).to(dt).float()
    return torch.bmm(v, w.permute(0, 2, 1))


def weights64(q, k, scale=None):
    """the softmax weights [B, query, key] in float64"""
    b, c = q.shape[:2]
    q, k = (t.detach().double().reshape(b, c, -1) for t in (q, k))
    return torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * _scale(c, scale), dim=2)


def e_model(ref64, q, k, v, scale=None):
    return max_err(model_expr(q, k, v, scale), ref64)[0]


def tiled_model(q, k, v, scale=None, guard=True):
    """the kernel's tile loop (csrc/cgic_attn.hip) in fp32 torch ops: tiles of ATTN_BK keys, a running maximum that ignores NaN (as
    v_max_f32 does), alpha 0 by a select while the maximum is still -inf, p = exp2((s - m) * scale * log2 e) rounded once to the
    operand type in front of the second product while the row sum adds the unrounded p, lse = m * scale + ln(l) in float64.
    guard=True subtracts 0 in place of a maximum that is still -inf (a leading tile whose scores are all -inf then weighs 0), and
    takes a weight or a rescale factor below 2^NEGLIGIBLE as exactly 0, as the kernel does (kNegligible);
    guard=False is the arithmetic before that fix: exp2(-inf - -inf) = NaN.  -> (out fp32 [B,C,N], lse fp32 [B,N])"""
    b, c = q.shape[:2]
    dt = q.dtype
    q, k, v = (t.detach().float().reshape(b, c, -1) for t in (q, k, v))
    n = q.shape[2]
    sc = float(_scale(c, scale))
    c2 = torch.tensor(sc * 1.4426950408889634, dtype=f32, device=q.device)
    s_all = torch.bmm(q.permute(0, 2, 1), k)                                    # [B, query, key], unscaled as in the kernel
    ninf = torch.tensor(-INF, dtype=f32, device=q.device)
    zero = torch.zeros((), dtype=f32, device=q.device)
    m = torch.full((b, n), -INF, dtype=f32, device=q.device)
    l = torch.zeros((b, n), dtype=f32, device=q.device)
    acc = torch.zeros((b, c, n), dtype=f32, device=q.device)
    for k0 in range(0, n, ATTN_BK):
        s = s_all[:, :, k0:k0 + ATTN_BK]
        mn = torch.maximum(m, torch.where(torch.isnan(s), ninf, s).amax(dim=2))
        ax = (m - mn) * c2
        alpha = torch.where(m == -INF, zero, torch.exp2(ax))
        sub = torch.where(mn == -INF, zero, mn) if guard else mn
        x = (s - sub[:, :, None]) * c2
        p = torch.exp2(x)
        if guard:                                                               # weights and rescales below 2^-64 are exact zeros
            alpha = torch.where(ax < NEGLIGIBLE, zero, alpha)
            p = torch.where(x < NEGLIGIBLE, zero, p)
        l = l * alpha + p.sum(dim=2)
        acc = acc * alpha[:, None, :] + torch.bmm(v[:, :, k0:k0 + ATTN_BK], p.to(dt).float().permute(0, 2, 1))
        m = mn
    return acc / l[:, None, :], (m.double() * sc + torch.log(l.double())).float()


def _neg(q):                    # queries whose planted-channel entry is negative: a +inf in k's channel scores -inf for them
    return q[0, C0].float() < 0


def _pos(q):
    return q[0, C0].float() > 0


def _queries(q, bad):
    """NaN at every channel of the queries `bad` of image 0"""
    nan = torch.zeros(q.shape, dtype=torch.bool)
    nan[0, :, bad] = True
    return nan


def _plant_k(lo, hi, value=INF):
    def plant(q, k, v):
        n = k.shape[2]
        k[0, C0, lo:(n + hi if hi is not None and hi <= 0 else hi)] = value
    return plant


def _plant_e(q, k, v):
    k[0, C0, 5] = INF
    k[0, C0, -1] = INF


def _plant_h(q, k, v):
    q[0, C0, 100] = INF


def _plant_j(q, k, v):
    q.zero_()
    v[0, 9, 200] = INF


def _plant_k2(q, k, v):
    _plant_j(q, k, v)
    v[0, 9, 10] = -INF


def _plant_offset(sign):
    def plant(q, k, v):
        q[0, C0, :] = sign * 200.0
        k[0, C0, :] = 200.0
    return plant


def _plant_ramp(slope):
    def plant(q, k, v):
        n = k.shape[2]
        q[0, 4:] = (q[0, 4:].float() * 0.1).to(q.dtype)
        k[0, 4:] = (k[0, 4:].float() * 0.1).to(k.dtype)
        q[0, 0:4, :] = 4.0
        k[0, 0:4, :] = (slope * torch.arange(n, dtype=f32)).to(k.dtype)
    return plant


def one_hot_winners(n):
    """the seeded permutation of case n: query i's weight is 1 on key winners[i]"""
    return torch.from_numpy(np.random.default_rng(4242 + n).permutation(n).astype(np.int64))


def _plant_n(q, k, v):
    q[0] = k[0][:, one_hot_winners(k.shape[2])] * 8


def _plant_o(q, k, v):
    q[0, C0, :] = 60000.0
    k[0, C0, ::3] = 0.25


def _nan_unless(sign_ok):
    return lambda q, k, v: {"nan": _queries(q, ~sign_ok(q))}


def _nan_all(q, k, v):
    nan = torch.zeros(q.shape, dtype=torch.bool)
    nan[0] = True
    return {"nan": nan}


def _nan_q100(q, k, v):
    bad = torch.zeros(q.shape[2], dtype=torch.bool)
    bad[100] = True
    return {"nan": _queries(q, bad)}


def _ch9(which):
    def expect(q, k, v):
        m = torch.zeros(q.shape, dtype=torch.bool)
        m[0, 9, :] = True
        return {which: m}
    return expect


_none = lambda q, k, v: {}

# name: (N, the widths C, the types, the scale (None: C ** -0.5), the planting in image 0, the expected non-finite patterns by index,
#        what the finite queries of image 0 must equal bit for bit: None, "last" v[:, :, N-1], "winners" v[:, :, winners])
_ALL = (f32, f16, bf16)
SCORE_CASES = {
    "a": (300, (256, 512), _ALL, None, _plant_k(0, 128), _nan_unless(_neg), None),
    "b": (300, (256,), _ALL, None, _plant_k(128, 256), _nan_unless(_neg), None),
    "c-N300": (300, (256, 512), _ALL, None, _plant_k(0, -1), _nan_unless(_neg), "last"),
    "c-N129": (129, (256, 512), _ALL, None, _plant_k(0, -1), _nan_unless(_neg), "last"),
    "d": (111, (256,), _ALL, None, _plant_k(0, None), _nan_all, None),
    "e": (300, (256,), _ALL, None, _plant_e, _nan_unless(_neg), None),
    "f": (300, (256,), _ALL, None, _plant_k(0, 127), _nan_unless(_neg), None),
    "g": (300, (256,), _ALL, None, _plant_k(0, 128, -INF), _nan_unless(_pos), None),
    "h": (300, (256,), _ALL, None, _plant_h, _nan_q100, None),
    "i": (300, (256,), _ALL, 0.0, _plant_k(0, 128), _nan_all, None),
    "j": (300, (256,), _ALL, None, _plant_j, _ch9("pinf"), None),
    "k": (300, (256,), _ALL, None, _plant_k2, _ch9("nan"), None),
    "l+N300": (300, (256, 512), _ALL, None, _plant_offset(1.0), _none, None),
    "l-N300": (300, (256, 512), _ALL, None, _plant_offset(-1.0), _none, None),
    "l+N6": (6, (256, 512), _ALL, None, _plant_offset(1.0), _none, None),
    "l-N6": (6, (256, 512), _ALL, None, _plant_offset(-1.0), _none, None),
    "m-slope2": (300, (256,), _ALL, None, _plant_ramp(2.0), _none, None),
    "m-slope0.02": (300, (256,), _ALL, None, _plant_ramp(0.02), _none, None),
    "m-slope-2": (300, (256,), _ALL, None, _plant_ramp(-2.0), _none, None),
    "n": (300, (256, 512), _ALL, None, _plant_n, _none, "winners"),
    "o": (300, (256,), (f16,), None, _plant_o, _none, None),
}
LEADING_INF_TILE = ("a", "c-N300", "c-N129", "g")      # the cases in which a leading key tile scores all -inf for some queries
SCORE_PARAMS = [(name, C, dt) for name, spec in SCORE_CASES.items() for C in spec[1] for dt in spec[2]]


class Built:
    """one case at one width and type, on the CPU: q, k, v [2,C,N] (image 0 planted, image 1 clean), the scale, the expected
    patterns (nan, pinf, ninf) and, where the case has one, (mask [N] of queries, expected [C, N]) for the bit equality"""


def build_case(name, C, dtype):
    N, _, _, scale, plant, expect, exact = SCORE_CASES[name]
    q, k, v = make_inputs(5 + 11 * sorted(SCORE_CASES).index(name) + C, 2, C, N, dtype)
    plant(q, k, v)
    c = Built()
    c.name, c.C, c.N, c.dtype, c.scale, c.q, c.k, c.v = name, C, N, dtype, scale, q, k, v
    e = expect(q, k, v)
    none = torch.zeros(q.shape, dtype=torch.bool)
    c.expect = tuple(e.get(key, none) for key in ("nan", "pinf", "ninf"))
    c.exact = None
    if exact == "last":
        c.exact = (_neg(q), v[0, :, -1:].expand(C, N))
    elif exact == "winners":
        c.exact = (torch.ones(N, dtype=torch.bool), v[0][:, one_hot_winners(N)])
    if name in "abcefg" or name[:2] == "c-":
        assert bool(_neg(q).any()) and bool(_pos(q).any()) and not bool((q[0, C0] == 0).any())     # both outcomes in the case
    if name == "n":
        assert {0, 127, 128, 255, 256, N - 1} <= set(one_hot_winners(N).tolist())
    return c


def case_refs(c, dev="cpu"):
    """the inputs of a built case on `dev` and what its results are held to, all computed there once:
    q, k, v, r64, l64, E_ref (NaN where torch's half chain overflows), E_model, rows (lse compared there), E_lse"""
    r = Built()
    r.q, r.k, r.v = (t.to(dev) for t in (c.q, c.k, c.v))
    r.r64 = restatement(r.q, r.k, r.v, c.scale)
    r.l64 = lse64(r.q, r.k, c.scale)
    r.e_ref = e_ref(r.r64, r.q, r.k, r.v, c.scale)
    r.e_model = e_model(r.r64, r.q, r.k, r.v, c.scale)
    # lse is a function of q and k alone: where v is finite, "the softmax row is finite" is "the row of the result is finite"
    w64 = weights64(r.q, r.k, c.scale)
    r.rows = torch.isfinite(r.l64) & torch.isfinite(w64).all(dim=2)
    r.runner_up = float(w64[0].topk(2, dim=1).values[:, 1].max()) if c.name == "n" else None     # (the largest second weight of a row)
    if bool(torch.isfinite(r.v).all()):
        assert torch.equal(r.rows, torch.isfinite(r.l64) & torch.isfinite(r.r64).all(dim=1))
    d = (lse_torch32(r.q, r.k, c.scale).double() - r.l64)[r.rows]
    r.e_lse = float(d.abs().max()) if d.numel() else 0.0
    return r


def judge(c, r, got32, lse, what, report=print):
    """every assertion of a case on a result (fp32 out [2,C,N], fp32 lse [2,N]); prints the figures first.  -> the ratios"""
    half = c.dtype != f32
    err = max_err(got32, r.r64)[0]
    bar1 = BAR_F32 if not half else BAR_HALF
    ratio = lambda e, unit: e / unit if unit else (0.0 if e == 0 else INF)
    dl = (lse.detach().double() - r.l64)[r.rows]
    err_lse = float(dl.abs().max()) if dl.numel() else 0.0
    out = {"ref": ratio(err, r.e_ref), "model": ratio(err, r.e_model), "lse": ratio(err_lse, r.e_lse)}
    report(f"{what}: err {err:.3e}  E_ref {r.e_ref:.3e} (ratio {out['ref']:.2f}, bar {bar1:g})  E_model {r.e_model:.3e} "
           f"(ratio {out['model']:.2f}, bar {BAR_F32:g})  lse err {err_lse:.3e}  E_lse {r.e_lse:.3e} (ratio {out['lse']:.2f}, bar {BAR_LSE:g})"
           f"  NaN {int(torch.isnan(got32[0]).any(dim=0).sum())} of {c.N} queries of image 0, the reference {int(torch.isnan(r.r64[0]).any(dim=0).sum())}")
    # 1. the patterns: the reference's, which are the ones spelled out by index
    assert same_patterns(r.r64, c.expect), (what, "the reference's patterns are not the documented ones")
    assert same_patterns(got32, c.expect), (what, "patterns")
    # 2. the values on the finite elements: the file's bar wherever torch's chain is finite, and 4 x the kernel's own precision model
    if r.e_ref == r.e_ref and r.e_ref != INF:
        assert err <= bar1 * r.e_ref, (what, "E_ref", err, r.e_ref)
    assert r.e_model == r.e_model and err <= BAR_F32 * r.e_model, (what, "E_model", err, r.e_model)
    # 3. lse: within the bar where the reference's lse and softmax row are finite, non-finite on every other row
    assert err_lse <= BAR_LSE * r.e_lse, (what, "lse", err_lse, r.e_lse)
    assert not bool(torch.isfinite(lse[~r.rows]).any()), (what, "lse is finite on a row whose reference is not")
    assert bool(torch.isfinite(lse[r.rows]).all()), (what, "lse is not finite on a row whose reference is")
    # 2, where the unit is 0: the finite queries of image 0 are v's own columns, bit for bit (last, so that a miss hides nothing else)
    if c.exact is not None:
        rows, want = c.exact
        rows, want = rows.to(got32.device), want.to(got32.device)
        differ = got32[0][:, rows] != want.float()[:, rows]
        assert not bool(differ.any()), (what, "bit equality", f"{int(differ.sum())} of {differ.numel()} elements differ")
    return out
