"""GPU: the fused attention (csrc/cgic_attn.hip) on infinite and saturated scores, against the float64 restatement of AttnBlock's
expression -- the regimes N(0,1) inputs never reach (tests/test_attention.py has the ordinary ones).

The catalogue is attention_ref.SCORE_CASES, generated from seeds; B = 2: image 0 carries the planting, image 1 is clean and must
come out with the bits of calling it alone.
  infinite scores   a +Inf (-Inf) in one channel of k scores -inf for every query whose q in that channel is negative (positive)
                    and +inf for the others: the first are finite in the reference (those keys weigh 0), the others NaN.  The
                    -inf keys cover a leading tile (a, c, g), a middle tile (b), all keys but the last (c: out is v[:, :, N-1] bit
                    for bit), every key (d: NaN), single keys (e), 127 of the first 128 (f); a +Inf in q (h); scale = 0 (i);
  infinite v        under uniform weights (q = 0): +Inf in a channel (j), +Inf and -Inf in it (k: NaN);
  saturated scores  a common offset of +-2500 (l: also the guard of the tail-key mask, whose zero scores would dominate a
                    negative offset), maxima that move by 256 nats per tile, by 2.5, or sit in the first tile (m), rows whose
                    weight is exactly 1 on one key at every position of a tile (n: out is v[:, :, winners] bit for bit), and a
                    fp16 q channel of 60000, where torch's half chain overflows (o).

What is asserted (attention_ref.judge, shared with the CPU tests of the tile loop's model in tests/test_attention_host.py):
  patterns   the NaN, the +Inf and the -Inf pattern of out each equal ref64's, and ref64's are the ones the case spells out by index;
  values     on the finite elements, err <= the file's existing bar x E_ref wherever E_ref is finite (fp32 4, half inputs 1), AND
             err <= 4 x E_model.  E_ref is the error of torch's chain in the operand type, which rounds the scores to the half type:
             at scores of +-2500 it is 0.23 to 3.7 and bounds nothing, and where that chain overflows (o) it is NaN.  E_model is the error of the kernel's own precision
             model in torch ops (fp32 scores from the exactly upcast inputs, fp32 softmax, weights rounded once to the operand type,
             fp32 second product): the same chain of roundings in another order, hence the project's margin of 4.  Where the unit is
             0 (c, n) the requirement is bit equality;
  lse        within 4 x the error of torch's fp32 logsumexp on the rows where lse64 and the reference's softmax row are finite
             (with finite v: where the row of ref64 is finite; lse does not depend on v), non-finite on every other row;
  half out   == .to(half) of the same call's fp32 out, bit for bit;
  module     cg.AttnBlock.adopt(StandIn) under autocast(fp16) with a k conv that overflows at the leading 128 tokens of image 0 (case
             a inside the block): the non-finite pattern of torch's path through the same module, which is the one spelled out.
Every test prints err, both units and the ratios before it asserts; the measured ratios are in profiles/attention.md.
"""
import pytest
import torch

import control_gic_amd as cg
import attention_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16

_cache = {}
_ids = [f"{name}-C{C}-{str(dt).split('.')[1]}" for name, C, dt in ref.SCORE_PARAMS]


def score_case(name, C, dtype):
    """(the built case, its inputs and references on the device): made once, shared, never changed"""
    key = (name, C, dtype)
    if key not in _cache:
        c = ref.build_case(name, C, dtype)
        _cache[key] = (c, ref.case_refs(c, DEV))
    return _cache[key]


@pytest.mark.parametrize("name,C,dtype", ref.SCORE_PARAMS, ids=_ids)
def test_the_catalogue_against_patterns_bars_and_lse(name, C, dtype):
    """Case n at C = 256 is the one that needs the kernel's kNegligible: before it, the fp32 out of half inputs was one fp32 ulp nearer
    zero at 3 (fp16) and 34 (bf16) of 76800 elements, because v_mfma_f32_32x32x16_{f16,bf16} returns the predecessor of v * 1 when v
    is a power of two and its C input is a non-zero number of the opposite sign, however small (profiles/attention.md)."""
    c, r = score_case(name, C, dtype)
    got32, lse = cg.attention(r.q, r.k, r.v, scale=c.scale, out_dtype=f32, lse=True)
    assert got32.dtype == f32 and got32.shape == r.q.shape and lse.dtype == f32 and lse.shape == (2, c.N)
    if name == "n":
        print(f"one-hot rows: the largest runner-up weight in float64 is {r.runner_up:.3e}")
        assert r.runner_up < 2.0 ** -60
    # the half out is the fp32 out rounded once; without lse the same bits
    own = cg.attention(r.q, r.k, r.v, scale=c.scale)
    assert own.dtype == dtype and ref.same_bits(own, got32.to(dtype))
    assert ref.same_bits(cg.attention(r.q, r.k, r.v, scale=c.scale, out_dtype=f32), got32)
    if c.exact is not None:
        rows, want = (t.to(DEV) for t in c.exact)
        assert torch.equal(own[0][:, rows], want[:, rows])                      # (in the operand type as well: v itself)
    # image 1 is clean: finite, and the bits of calling it alone
    one, lse1 = cg.attention(r.q[1:], r.k[1:], r.v[1:], scale=c.scale, out_dtype=f32, lse=True)
    assert bool(torch.isfinite(got32[1]).all()) and torch.equal(one[0], got32[1]) and torch.equal(lse1[0], lse[1])
    ref.judge(c, r, got32, lse, f"{name} C{C} {dtype}")


def _overflowing_block(C, seed):
    """a stand-in of the reference's block whose k conv overflows fp16 under autocast as catalogue case a does: tokens 0..127 of
    image 0 carry an outlier in input channel 3, which the block's GroupNorm turns into about +4 there and -0.25 elsewhere, and
    row C0 of the k conv reads that channel with a weight of 20000 -- about +85000 (Inf in fp16) at those tokens, about -5000 at the
    others.  Checked here on the CPU in fp32, not by trial on the device."""
    with torch.random.fork_rng(devices=[]):                                      # (the initial parameters come from the global generator:
        torch.manual_seed(seed)                                                  #  the same block whatever ran before, and nothing after sees it)
        theirs = ref.randomize(ref.StandIn(C), seed).eval()
    x = torch.randn(2, C, 10, 30, generator=torch.Generator().manual_seed(seed + 1))
    x[0, 3].view(-1)[:ref.ATTN_BK] += 100.0
    x[1, 3] *= 0.05                                                              # (the clean image: that channel small against its group)
    with torch.no_grad():
        theirs.k.weight[ref.C0].zero_()
        theirs.k.weight[ref.C0, 3] = 20000.0
        theirs.k.bias[ref.C0] = 0.0
        k = theirs.k(theirs.norm(x)).reshape(2, C, -1)
        q = theirs.q(theirs.norm(x)).reshape(2, C, -1)
    top = 65520.0                                                                # what rounds to Inf in fp16
    over = k > top
    want = torch.zeros_like(over)
    want[0, ref.C0, :ref.ATTN_BK] = True
    assert torch.equal(over, want) and float(k[~over].abs().max()) < 10000.0 and float(k[over].min()) > 1.1 * top
    # the scores of the finite keys stay inside fp16 in torch's half chain: |q k| summed over the channels
    assert float(torch.bmm(q.abs().permute(0, 2, 1), torch.where(over, torch.zeros_like(k), k).abs()).max()) < 0.75 * top
    assert 100 < int((q[0, ref.C0] < 0).sum()) < 200                             # both outcomes among the 300 queries
    # ... and none so near 0 that the half conv's rounding could turn its sign, or that it is a fp16 subnormal (below 6.1e-5) which a
    # matrix unit may flush to 0, making 0 * inf of it
    assert float(q[0, ref.C0].abs().min()) > 1e-3
    return theirs, x


def test_the_module_under_autocast_fp16_with_an_overflowing_k_conv():
    """cg.AttnBlock.adopt(StandIn) under autocast(fp16) where the k conv overflows to +Inf in channel C0 at the 128 leading tokens
    of image 0 (catalogue case a inside the module): the non-finite pattern of the block's output is that of torch's path through
    the same module, and it is the one spelled out: every channel of the queries of image 0 whose q in that channel is not negative"""
    theirs, x = _overflowing_block(256, 21)
    theirs, x = theirs.to(DEV), x.to(DEV)
    mine = cg.AttnBlock.adopt(theirs)
    seen = {}
    # The half conv of this stack converts its fp32 sums to fp16 toward zero: where the sum overflows it returns the largest fp16
    # (65504.0 measured on MI355X at these very elements), not Inf.  A conv that rounds to nearest returns Inf there, and that is
    # the regime under test, so a hook on the shared k conv -- both paths run it -- turns what saturated into what overflowed.
    to_nearest = lambda m, a, res: torch.where(res.abs() >= 65504.0, res * 2, res)
    hooks = [mine.k.register_forward_hook(to_nearest)]
    hooks += [getattr(mine, n).register_forward_hook(lambda m, a, res, n=n: seen.__setitem__(n, res.detach())) for n in ("q", "k")]
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=f16):
            assert mine.uses_kernel(*(mine.q(x),) * 3) and mine.q(x).dtype == f16
            y_torch = theirs(x)
            y_mine = mine(x)
    finally:
        for h in hooks:
            h.remove()
    q, k = (seen[n].reshape(2, 256, -1) for n in ("q", "k"))
    expect_k = torch.zeros_like(k, dtype=torch.bool)
    expect_k[0, ref.C0, :ref.ATTN_BK] = True
    assert k.dtype == f16 and torch.equal(k == ref.INF, expect_k) and bool(torch.isfinite(k[~expect_k]).all())
    finite_queries = q[0, ref.C0] < 0                                            # (of the fp16 q the conv returned)
    expect = torch.zeros(x.shape, dtype=torch.bool, device=DEV).view(2, 256, -1)
    expect[0, :, ~finite_queries] = True
    n_mine, n_torch = (int(torch.isnan(y[0]).any(dim=0).sum()) for y in (y_mine.view(2, 256, -1), y_torch.view(2, 256, -1)))
    print(f"module autocast(fp16), k conv overflowing: NaN at {n_mine} of 300 queries of image 0, torch's path at {n_torch}, spelled out {int((~finite_queries).sum())}")
    assert y_mine.dtype == y_torch.dtype and y_mine.shape == y_torch.shape
    assert ref.same_patterns(y_torch, (expect.view(x.shape), torch.zeros_like(expect).view(x.shape), torch.zeros_like(expect).view(x.shape)))
    assert ref.same_patterns(y_mine, y_torch)
