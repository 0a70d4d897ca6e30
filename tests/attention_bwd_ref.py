"""What the tests of the attention's backward pass (csrc/cgic_attn_bwd.hip) measure against, on whichever device the inputs are.
One image is [C, N]: the first index is the channel, the second the query or key.  With s_ij = scale * sum_c q[c,i] k[c,j]:

    P_ij = exp(s_ij - lse_i)    delta_i = sum_c go[c,i] out[c,i]    dP_ij = sum_c go[c,i] v[c,j]    dS_ij = P_ij (dP_ij - delta_i)
    dv[c,j] = sum_i go[c,i] P_ij      dq[c,i] = scale sum_j dS_ij k[c,j]      dk[c,j] = scale sum_i dS_ij q[c,i]

  grads64(go, q, k, v)      float64 autograd of attention_ref.restatement's expression from the exactly upcast inputs: the reference;
  formulas64(go, q, k, v)   the seven formulas above written out in float64 (held to grads64 by tests/test_attention_bwd_host.py);
  grads_torch(go, q, k, v)  autograd through attention_ref.torch_expr's chain in the operand type, not detached -- what the module's
                            torch path computes today (for halves: as under autocast).  Its max-abs error against grads64 is E_ref;
  grads_model(go, q, k, v)  the kernels' precision model in fp32 torch ops; its max-abs error against grads64 is E_model.

The precision model, once:
  - scores s and dP are fp32 sums of the exactly upcast inputs;
  - lse is the forward's: ln sum_j exp(scale * s_ij) from fp32 scores, evaluated in float64 and rounded once to fp32;
    out is the forward's model (attention_ref.model_expr) rounded once to the operand type;
  - P = exp2((s * scale - lse) * log2 e) in fp32, scale and log2 e as fp32 numbers; an exponent below NEGLIGIBLE (the forward's
    kNegligible) gives an exact 0;
  - tail keys and tail queries are zeros by a select, never 0 * x (the model has no tails: it works on whole rows);
  - delta is an fp32 sum of the fp32 products go * out;
  - P and dS are rounded once to the operand type in front of the second products, which accumulate in fp32;
  - scale is applied once, in fp32, to the finished sums of dq and dk; a half result is the fp32 one rounded once.
`perm` (a permutation of the channels) reorders every sum over the channels -- scores, dP and delta --: a stand-in for the kernel's
own summation order, which no torch expression reproduces.

N = 1 has known answers, dv = go and dq = dk = 0, and the units above say nothing there (both are rounding noise around 0).  The caps:
  dv:  P = exp2((s * scale - lse) * log2 e) with lse = fl(s * scale) from the forward.  The two evaluations of s * scale (fp32 in the
       backward, float64 rounded once in the forward; the fp32 scale itself is the double one rounded) differ by at most
       2^-23 |lse|, the exponent's own roundings and exp2's add at most 2^-23, and go * P rounds once more below that:
       |dv - go| <= 2^-22 * max(1, |lse|) * |go|.  For halves P rounds to exactly 1 and dv = go.
  dq, dk:  dS = P (dP - delta) with dP = sum_c go_c v_c and delta = sum_c go_c out_c, out = v (one key of weight 1: the forward
       returns v's bits).  The two are the same sum in two orders of C terms: each within C * 2^-24 * sum_c |go_c v_c| of the exact
       sum, so |dS| <= 2 * C * 2^-24 * sum_c |go_c v_c| * P, and P <= 2:  |dq|, |dk| <= scale * max|k or q| * 4 * C * 2^-24 * sum_c |go_c v_c|.
"""
import numpy as np
import torch

import attention_ref as ref

f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
GRADS = ("dq", "dk", "dv")
LOG2E = 1.4426950408889634
BAR_F32 = ref.BAR_F32          # 4: x max(E_ref, E_model) for fp32 inputs, and x E_model for halves
BAR_HALF = ref.BAR_HALF        # 1: x E_ref for halves -- not worse than what it replaces
NEGLIGIBLE = ref.NEGLIGIBLE

# name: (N, what is done to the seeded N(0,1) inputs) -- the smallest shapes at which each part of the kernels can go wrong
CASES = {
    "N1": (1, None),                    # one token
    "N6": (6, None),                    # fewer than any tile
    "N111": (111, None),                # odd: unaligned rows, ragged query and key tails
    "N256": (256, None),                # whole tiles
    "N300-q4": (300, "gain4"),          # q x 4: moving maxima in the forward, peaked rows here
    "N300-onehot": (300, "onehot"),     # image 0: q = 8 * k[:, perm], one weight of 1 per row
    "N1776": (1776, None),              # 37 x 48: many tiles, ragged last
    "N111-q0": (111, "q0"),             # q = 0: dk is exactly 0
}
WIDTHS = (256, 512)
BATCHES = (1, 3)
TYPES = (f32, f16, bf16)
# The catalogue of the GPU test is every (case, C, B, type) except the entries below, on which the precision model ALONE -- on the
# CPU, before any kernel ran: tests/test_attention_bwd_host.py::test_feasibility -- misses the half bar err <= 1 * E_ref:
#   N6 in bf16: 6 x C elements per image, E_ref is the maximum of a sample that small, and the model's dS, rounded to bf16 like
#       torch's, lands at 1.1 to 1.3 x that;
#   one-hot rows at B = 1 in the half types: every row has one weight of 1, torch's softmax backward returns dq and dk of 1e-32
#       there (E_ref is no unit any more), the model's delta cancels against dP at 5e-6.  At B = 3 images 1 and 2 are ordinary.
# The host test also asserts that each of them does miss, so that the catalogue is the widest set that is feasible.
EXCLUDED = {("N6", 256, 1, bf16), ("N6", 256, 3, bf16), ("N6", 512, 3, bf16),
            ("N300-onehot", 256, 1, f16), ("N300-onehot", 256, 1, bf16), ("N300-onehot", 512, 1, f16), ("N300-onehot", 512, 1, bf16)}
# N1 is held to its own caps (n1_caps), not to the units
CATALOGUE = [(name, C, B, dt) for name in CASES for C in WIDTHS for B in BATCHES for dt in TYPES if (name, C, B, dt) not in EXCLUDED]
FEASIBILITY_PERMS = 3


def perms(name, C):
    """the seeded channel permutations of the feasibility check"""
    g = torch.Generator().manual_seed(C + CASES[name][0])
    return [torch.randperm(C, generator=g) for _ in range(FEASIBILITY_PERMS)]


def _scale(c, scale):
    return int(c) ** (-0.5) if scale is None else scale


def make_case(name, B, C, dtype):
    """go, q, k, v [B,C,N] of `dtype`, seeded, on the CPU"""
    N, how = CASES[name]
    seed = 7000 + 31 * sorted(CASES).index(name) + C + B
    q, k, v = ref.make_inputs(seed, B, C, N, dtype, gain=4.0 if how == "gain4" else 1.0)
    if how == "onehot":
        q[0] = (k[0].float()[:, ref.one_hot_winners(N)] * 8).to(dtype)             # (image 0, as attention_ref.SCORE_CASES["n"])
    elif how == "q0":
        q = torch.zeros_like(q)
    go = torch.from_numpy(np.random.default_rng(seed + 1).standard_normal((B, C, N)).astype(np.float32)).to(dtype)
    return go, q, k, v


def grads64(go, q, k, v, scale=None):
    """(dq, dk, dv) float64 [B,C,N]: autograd of the reference's expression from the exactly upcast inputs"""
    b, c = q.shape[:2]
    q, k, v = (t.detach().double().reshape(b, c, -1).requires_grad_() for t in (q, k, v))
    w = torch.bmm(q.permute(0, 2, 1), k) * _scale(c, scale)
    w = torch.softmax(w, dim=2)
    out = torch.bmm(v, w.permute(0, 2, 1))
    return torch.autograd.grad(out, (q, k, v), go.detach().double().reshape(b, c, -1))


def formulas64(go, q, k, v, scale=None):
    """the seven formulas of the head of this file, in float64"""
    b, c = q.shape[:2]
    go, q, k, v = (t.detach().double().reshape(b, c, -1) for t in (go, q, k, v))
    sc = _scale(c, scale)
    s = torch.einsum("bci,bcj->bij", q, k) * sc
    lse = torch.logsumexp(s, dim=2)
    p = torch.exp(s - lse[:, :, None])
    out = torch.einsum("bcj,bij->bci", v, p)
    delta = (go * out).sum(dim=1)
    dp = torch.einsum("bci,bcj->bij", go, v)
    ds = p * (dp - delta[:, :, None])
    return sc * torch.einsum("bij,bcj->bci", ds, k), sc * torch.einsum("bij,bci->bcj", ds, q), torch.einsum("bci,bij->bcj", go, p)


def grads_torch(go, q, k, v, scale=None):
    """(dq, dk, dv) in the operand type: autograd through torch_expr's chain (halves: the chain autocast makes of the module's
    expression -- bmm in the half type, the scale in the half type, softmax in fp32, the weights cast to the half type, bmm)"""
    b, c = q.shape[:2]
    q, k, v = (t.detach().reshape(b, c, -1).requires_grad_() for t in (q, k, v))
    w = torch.bmm(q.permute(0, 2, 1), k)
    w = w * _scale(c, scale)
    w = torch.softmax(w.float(), dim=2).to(q.dtype)
    out = torch.bmm(v, w.permute(0, 2, 1))
    return torch.autograd.grad(out, (q, k, v), go.detach().reshape(b, c, -1))


def grads_model(go, q, k, v, scale=None, perm=None):
    """(dq, dk, dv) fp32: the precision model of the head of this file.  perm: a permutation of the channels under which every sum
    over the channels is taken (the results come back in the channels' own order)"""
    b, c = q.shape[:2]
    dt = q.dtype
    go, q, k, v = (t.detach().reshape(b, c, -1) for t in (go, q, k, v))
    if perm is not None:
        go, q, k, v = (t[:, perm] for t in (go, q, k, v))
    out = ref.model_expr(q, k, v, scale).to(dt).float()
    go, q, k, v = (t.float() for t in (go, q, k, v))
    sc = torch.tensor(_scale(c, scale), dtype=f32, device=q.device)
    s = torch.bmm(q.permute(0, 2, 1), k)                                               # [B, query, key], unscaled as in the kernel
    lse = torch.logsumexp(s.double() * float(_scale(c, scale)), dim=2).float()
    x = (s * sc - lse[:, :, None]) * torch.tensor(LOG2E, dtype=f32, device=q.device)
    p = torch.where(x < NEGLIGIBLE, torch.zeros((), dtype=f32, device=q.device), torch.exp2(x))
    delta = (go * out).sum(dim=1)
    dp = torch.bmm(go.permute(0, 2, 1), v)
    ds = (p * (dp - delta[:, :, None])).to(dt).float()
    p = p.to(dt).float()
    dq, dk, dv = sc * torch.bmm(k, ds.permute(0, 2, 1)), sc * torch.bmm(q, ds), torch.bmm(go, p)
    if perm is not None:
        inv = torch.argsort(perm)
        dq, dk, dv = dq[:, inv], dk[:, inv], dv[:, inv]
    return dq, dk, dv


def errors(got, g64):
    """{name: max-abs error against the float64 gradient}"""
    return {n: ref.max_err(g, r)[0] for n, g, r in zip(GRADS, got, g64)}


class Refs:
    """the inputs of a case on a device and what its results are held to, all computed there once: go, q, k, v, g64 (the three
    float64 gradients), e_ref and e_model ({name: unit})"""


def case_refs(go, q, k, v, scale=None, dev="cpu"):
    r = Refs()
    r.go, r.q, r.k, r.v = (t.to(dev) for t in (go, q, k, v))
    r.scale = scale
    r.g64 = grads64(r.go, r.q, r.k, r.v, scale)
    r.e_ref = errors(grads_torch(r.go, r.q, r.k, r.v, scale), r.g64)
    r.e_model = errors(grads_model(r.go, r.q, r.k, r.v, scale), r.g64)
    return r


def bars(r):
    """{name: (the bar on the max-abs error of a fp32 gradient, the text of how it came about)}"""
    out = {}
    for n in GRADS:
        if r.q.dtype == f32:
            out[n] = BAR_F32 * max(r.e_ref[n], r.e_model[n])
        else:
            out[n] = min(BAR_HALF * r.e_ref[n], BAR_F32 * r.e_model[n])
    return out


def judge(r, got32, what, names=GRADS, report=print):
    """every assertion on fp32 gradients (a dict name -> tensor, or a tuple in GRADS' order); prints the ratios first.
    fp32 inputs: err <= 4 * max(E_ref, E_model); halves: err <= 1 * E_ref and err <= 4 * E_model; a bar of 0 asks for exact zeros"""
    if not isinstance(got32, dict):
        got32 = dict(zip(GRADS, got32))
    bar = bars(r)
    ratio = lambda e, unit: e / unit if unit else (0.0 if e == 0 else float("inf"))
    rows = []
    for n in names:
        err, same_nan = ref.max_err(got32[n], r.g64[GRADS.index(n)])
        rows.append((n, err, same_nan))
    report(what + ": " + "  ".join(f"{n} err {err:.2e} /E_ref {ratio(err, r.e_ref[n]):.2f} /E_model {ratio(err, r.e_model[n]):.2f}" for n, err, _ in rows))
    for n, err, same_nan in rows:
        assert same_nan, (what, n, "NaN pattern")
        assert err <= bar[n], (what, n, err, "E_ref", r.e_ref[n], "E_model", r.e_model[n])
    return {n: (ratio(err, r.e_ref[n]), ratio(err, r.e_model[n])) for n, err, _ in rows}


def n1_caps(go, q, k, v, lse, scale=None):
    """N = 1: the absolute caps on |dv - go|, |dq| and |dk| derived in the head of this file, each [B,C,1] float64"""
    b, c = q.shape[:2]
    go, q, k, v = (t.detach().double().reshape(b, c, 1) for t in (go, q, k, v))
    sc = float(_scale(c, scale))
    cap_v = 2.0 ** -22 * torch.clamp(lse.detach().double().abs().reshape(b, 1, 1), min=1.0) * go.abs()
    noise = 4 * c * 2.0 ** -24 * (go * v).abs().sum(dim=1, keepdim=True)
    return cap_v, sc * k.abs().amax(dim=1, keepdim=True) * noise * torch.ones_like(q), sc * q.abs().amax(dim=1, keepdim=True) * noise * torch.ones_like(k)


# NaN planted at one element of image 0 of [2,C,300]: (the tensor, the element) -> the NaN pattern of image 0 of each gradient, by
# index; image 1 stays clean.  "all": the whole image, "none": nothing, ("col", i): [:, i], ("row", c): [c, :]
C0, I0 = 7, 100
NAN_CASES = {
    "go": {"dq": ("col", I0), "dk": "all", "dv": ("row", C0)},
    "q": {"dq": ("col", I0), "dk": "all", "dv": "all"},
    "k": {"dq": "all", "dk": "all", "dv": "all"},
    "v": {"dq": "all", "dk": "all", "dv": "none"},
}


def nan_case(which, C, dtype, N=300):
    """go, q, k, v [2,C,N] with a NaN at [0, C0, I0] of `which`"""
    t = dict(zip(("go", "q", "k", "v"), make_case("N300-q4", 2, C, dtype)))
    assert t["q"].shape[2] == N
    t[which][0, C0, I0] = float("nan")
    return t["go"], t["q"], t["k"], t["v"]


def nan_pattern(spec, C, N):
    """the expected NaN mask [2,C,N] of one gradient"""
    m = torch.zeros((2, C, N), dtype=torch.bool)
    if spec == "all":
        m[0] = True
    elif spec != "none":
        if spec[0] == "col":
            m[0, :, spec[1]] = True
        else:
            m[0, spec[1], :] = True
    return m
