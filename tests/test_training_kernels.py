"""The kernels of the reference's training graph and of the decoder's feature path at their edges: the VQ backward
(csrc/cgic_vq_bwd.hip) and the merge / pool / blend streams on fp32 features (csrc/cgic_merge.hip) against references computed ON THE CPU
(numpy fp32 / fp64, or the reference's own expressions on torch CPU tensors), plus the argument checks of their wrappers.

The VQ backward's codebook gradient is held to a bound DERIVED from the documented scheme (cgic_vq_bwd.hip): every workgroup
takes a range of vectors, quantises each difference to 2^(e_M - 30) (e_M: exponent of the range's largest finite |e - z|) by
round-to-nearest, sums integers, and the ranges' tables are added as doubles in range order; one fp32 rounding at the end.
A term is therefore off by at most half a quantum, 2^(e_M - 31):

    |gw[k] - want[k]| <= |ce| * sum_j count(range j, code k) * 2^(e_M_j - 31)  +  2^-23 * |want[k]|

(2^-24 of the second term is the final fp32 rounding, the rest covers the double additions).  `test_the_bound_is_not_vacuous`
runs a numpy emulation of that arithmetic and two broken variants of it against the bound on the CPU."""
import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd.quantize import vq_backward

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
BETA = 0.25


# ---------------------------------------------------------------------------- VQ backward: reference, bound, emulation (CPU)
def bwd_ranges(N):
    """the launch as documented: min(256, ceil(N / 2048)) workgroups, ceil(N / workgroups) consecutive vectors each
    (recomputed here, never asked from the library)"""
    nblk = max(1, min(256, -(-N // 2048)))
    per = -(-N // nblk)
    return [(j * per, min(N, (j + 1) * per)) for j in range(nblk) if j * per < N]


def flat(z):
    """[B,4,h,w] -> [N,4], vector n = (b, y, x)"""
    return np.ascontiguousarray(z.transpose(0, 2, 3, 1)).reshape(-1, 4)


def unflat(zf, B, h, w):
    return np.ascontiguousarray(zf.reshape(B, h, w, 4).transpose(0, 3, 1, 2))


def bwd_reference(z, cb, idx, g_zq, g_loss, legacy):
    """(d [N,4] fp32, ce fp32, want_gz [B,4,h,w] fp32, want_gw [K,4] fp64): the header's expressions, fp32 operation by fp32
    operation for g_z, the row sums in fp64 for the codebook"""
    B, _, h, w = z.shape
    N = B * h * w
    with np.errstate(all="ignore"):
        d = cb[idx] - flat(z)                                             # fp32, IEEE: the kernel's bits
        w_z, w_e = (1.0, BETA) if legacy else (BETA, 1.0)
        scale = 2.0 / (N * 4.0)
        coef_z, coef_e = F32(-scale * w_z), F32(scale * w_e)
        gl = F32(0.0 if g_loss is None else g_loss)
        cz, ce = gl * coef_z, gl * coef_e                                 # fp32 products
        assert cz.dtype == F32 and ce.dtype == F32
        m = unflat(cz * d, B, h, w)
        want_gz = m if g_zq is None else g_zq + m
        assert want_gz.dtype == F32
        sums = np.stack([np.bincount(idx, weights=d[:, c].astype(F64), minlength=cb.shape[0]) for c in range(4)], axis=1)
        want_gw = F64(ce) * sums
    return d, ce, want_gz, want_gw


def range_scale(d):
    """(q, largest error of one term) of a range with M = its largest FINITE |d|: the differences are rounded to multiples of
    2^-q, q = 30 - e_M.  M = 0: nothing to round.  M subnormal: the kernel's quantum is 1, every term (below 2^-126) is dropped."""
    a = np.abs(d)
    a = a[np.isfinite(a)]
    M = F32(a.max()) if a.size else F32(0)
    if M < np.finfo(F32).tiny:
        return 0, (0.0 if M == 0 else 2.0 ** -126)
    e = int(np.frexp(M)[1]) - 1
    return 30 - e, 2.0 ** (e - 31)


def gw_bound(d, idx, K, ce, want_gw):
    tol = np.zeros((K, 1), F64)
    for lo, hi in bwd_ranges(len(idx)):
        tol[:, 0] += np.bincount(idx[lo:hi], minlength=K) * range_scale(d[lo:hi])[1]
    with np.errstate(all="ignore"):
        return abs(F64(ce)) * tol + 2.0 ** -23 * np.abs(want_gw)


def emulate_gw(d, idx, K, ce, drop_last_of=None, coarser=0, global_max=False):
    """the documented arithmetic in numpy (finite differences only); the keyword arguments break it on purpose"""
    s = np.zeros((K, 4), F64)
    for j, (lo, hi) in enumerate(bwd_ranges(len(idx))):
        q = range_scale(d if global_max else d[lo:hi])[0]
        q -= coarser if q else 0
        if j == drop_last_of:
            hi -= 1
        v = np.rint(np.ldexp(d[lo:hi].astype(F64), q))                    # integers below 2^31: exact in a double
        acc = np.stack([np.bincount(idx[lo:hi], weights=v[:, c], minlength=K) for c in range(4)], axis=1)   # sums below 2^53: exact
        s += np.ldexp(acc, -q)
    return (F64(ce) * s).astype(F32)


class Case:
    def __init__(self, kind, B, h, w, K, seed=0):
        rng = np.random.default_rng([seed, B, h, w, K])
        N = B * h * w
        self.kind, self.B, self.h, self.w, self.K, self.N = kind, B, h, w, K, N
        self.cb = rng.standard_normal((K, 4)).astype(F32)
        zf = rng.standard_normal((N, 4)).astype(F32)
        idx = rng.integers(0, K, N)
        if kind in ("one_code", "one_code_centred"):                      # worst LDS contention, largest sums
            idx[:] = K - 1
            if kind == "one_code_centred":                                # the vectors scatter AROUND their code: the sum is ~sqrt(N)
                zf += self.cb[K - 1]
        elif kind == "on_code":                                           # M = 0 in every range
            zf = self.cb[idx].copy()
        elif kind == "subnormal_range":                                   # the last range holds subnormal differences only
            lo = bwd_ranges(N)[-1][0]
            idx[:lo], idx[lo:] = idx[:lo] % (K // 2), K // 2 + idx[lo:] % (K // 2)
            self.cb[K // 2:] = (self.cb[K // 2:].astype(F64) * 1e-40).astype(F32)
            zf[lo:] = (zf[lo:].astype(F64) * 1e-40).astype(F32)
        elif kind in ("range_within", "range_across"):
            # one outlier |d| ~ 2^20 in the first range; row `r` only has members with |d| < 2^-12, all of them in the LAST range
            r, last = 5, bwd_ranges(N)[-1]
            idx[idx == r] = r + 1
            self.tiny = last[0] + rng.choice(last[1] - last[0], 40, replace=False)
            self.tiny = self.tiny[self.tiny != 0]
            idx[self.tiny] = r
            zf[self.tiny] = self.cb[r] + (rng.uniform(0.5, 1.0, (len(self.tiny), 4)) * 2.0 ** -13).astype(F32)
            zf[0, 1] = self.cb[idx[0], 1] - F32(2.0 ** 20)
            self.row = r
        self.idx = idx
        self.z = unflat(zf, B, h, w)
        self.g_zq = rng.standard_normal(self.z.shape).astype(F32)


def _check_range_case(c, d):
    assert np.abs(d[c.tiny]).max() < 2.0 ** -12 and np.abs(d[c.tiny]).min() > 2.0 ** -15 and set(np.flatnonzero(c.idx == c.row)) == set(c.tiny)
    assert 2.0 ** 19 < np.abs(d[0]).max() < 2.0 ** 21
    assert len(bwd_ranges(c.N)) == (1 if c.kind == "range_within" else 2)


def test_the_bound_is_not_vacuous():
    """CPU: the emulation of the documented arithmetic meets the bound on random data, on one code and on both dynamic-range
    cases; an emulation that drops the last vector of one range, one with a 2^10 coarser quantum and one that takes the quantum
    from the global maximum do not."""
    assert bwd_ranges(1) == [(0, 1)] and bwd_ranges(2049) == [(0, 1025), (1025, 2049)]
    assert [hi - lo for lo, hi in bwd_ranges(4097)] == [1366, 1366, 1365]
    r = bwd_ranges(526337)
    assert len(r) == 256 and r[0] == (0, 2057) and r[-1] == (255 * 2057, 526337)
    for c in (Case("randn", 4, 32, 32, 1024), Case("one_code", 2, 64, 40, 16), Case("one_code_centred", 2, 64, 40, 16),
              Case("range_within", 2, 32, 32, 64), Case("range_across", 4, 32, 32, 64), Case("subnormal_range", 4, 32, 32, 64)):
        d, ce, _, want = bwd_reference(c.z, c.cb, c.idx, None, 3.0, True)
        bound = gw_bound(d, c.idx, c.K, ce, want)
        err = lambda **kw: np.abs(emulate_gw(d, c.idx, c.K, ce, **kw).astype(F64) - want)
        assert (err() <= bound).all(), c.kind
        if c.kind == "subnormal_range":                                   # documented: such a range contributes zero
            assert 0 < np.abs(d[2048:]).max() < np.finfo(F32).tiny and want[32:].any() and not emulate_gw(d, c.idx, c.K, ce)[32:].any()
            continue
        if c.kind.startswith("range"):
            _check_range_case(c, d)
            if c.kind == "range_across":                                  # the tiny row is held to ITS range's quantum
                assert (bound[c.row] < 1e-3 * np.abs(want[c.row])).all()
                assert not (err(global_max=True) <= bound).all()
        for j in (0, len(bwd_ranges(c.N)) - 1):
            assert not (err(drop_last_of=j) <= bound).all(), (c.kind, j)
        # on one code with sums of order N the row's own 2^-23 |want| exceeds even the coarse quantum's error: there the
        # coarse quantum is held against the bound with the vectors centred on their code
        if c.kind != "one_code":
            assert not (err(coarser=10) <= bound).all(), c.kind


# ---------------------------------------------------------------------------- VQ backward on the GPU
def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_bwd(c, g_loss=3.0, g_zq=True, legacy=True, want_gz=True, want_gw=True, z=None):
    gl = None if g_loss is None else torch.tensor(g_loss, dtype=torch.float32, device="cuda")
    gz, gw = vq_backward(_dev(c.z if z is None else z), _dev(c.cb), _dev(c.idx), _dev(c.g_zq) if g_zq else None, gl, BETA, legacy,
                         want_gz=want_gz, want_gw=want_gw)
    torch.cuda.synchronize()
    return (None if gz is None else gz.cpu().numpy()), (None if gw is None else gw.cpu().numpy())


def assert_same_bits(got, want):
    """NaNs in the same places, the same bit patterns everywhere else"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == F32 and want.dtype == F32 and got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{int((gn != wn).sum())} NaN positions differ"
    diff = (got.view(np.int32) != want.view(np.int32)) & ~wn
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} bit patterns differ, first at {np.argwhere(diff)[0]}"


def assert_gw_within_bound(gw, d, c, ce, want, where=None):
    bound = gw_bound(d, c.idx, c.K, ce, want)
    with np.errstate(all="ignore"):
        bad = ~(np.abs(gw.astype(F64) - want) <= bound)
    if where is not None:
        bad &= where
    worst = np.argwhere(bad)[0] if bad.any() else None
    assert not bad.any(), (f"{int(bad.sum())} components outside the bound, e.g. {worst}: got {gw[tuple(worst)]!r}, "
                           f"want {want[tuple(worst)]!r}, bound {bound[tuple(worst)]!r}")


def check_bwd(c, g_loss=3.0, g_zq=True, legacy=True):
    d, ce, want_gz, want_gw = bwd_reference(c.z, c.cb, c.idx, c.g_zq if g_zq else None, g_loss, legacy)
    gz, gw = run_bwd(c, g_loss, g_zq, legacy)
    assert_same_bits(gz, want_gz)
    assert_gw_within_bound(gw, d, c, ce, want_gw)
    assert_same_bits(gw, emulate_gw(d, c.idx, c.K, ce))                   # the documented arithmetic, to the bit
    return gz, gw


BIG = (7, 75191, 1)          # 526 337 = 257 * 2048 + 1 vectors: the 256-workgroup cap, 2057 per range (last one 1802), images of 75 191
SHAPES = [  # B, h, w, K
    (1, 1, 1, 1024),         # a single vector
    (5, 3, 17, 16),          # 255
    (1, 16, 16, 1000),       # 256; K not a multiple of the 256 staging threads
    (257, 1, 1, 1),          # 257, hw = 1, every vector on the only code
    (3, 683, 1, 2048),       # 2049: two ranges of 1025 / 1024 that cross the images; 96 KB of LDS
    (4097, 1, 1, 1024),      # three ranges of 1366 / 1366 / 1365, hw = 1
    (1, 11, 1, 16),
    BIG + (1000,),
    BIG + (2048,),
]


@gpu
@pytest.mark.parametrize("legacy", [True, False])
@pytest.mark.parametrize("B,h,w,K", SHAPES)
def test_vq_backward_random_data_at_every_launch_shape(B, h, w, K, legacy):
    """(a) g_z bit-identical to g_zq + cz * d, g_codebook within the derived bound and equal to the emulation"""
    check_bwd(Case("randn", B, h, w, K), legacy=legacy)


@gpu
def test_vq_backward_refuses_a_codebook_beyond_2048_rows():
    c = Case("randn", 1, 4, 4, 2049)
    with pytest.raises(cg.CgicError, match=r"K<=2048"):
        run_bwd(c)


@gpu
def test_vq_backward_every_vector_on_one_code_at_the_capped_grid():
    """(b): 526 337 vectors on one row -- every LDS atomic of a workgroup lands on four addresses; sums of order 1e6"""
    check_bwd(Case("one_code", *BIG, 1024))


@gpu
def test_vq_backward_z_on_its_code_gives_exact_zeros():
    """(c) M = 0 in every range: g_codebook is exactly zero and g_z is g_zq"""
    c = Case("on_code", 3, 683, 1, 1000)
    gz, gw = check_bwd(c)
    assert not gw.any() and np.array_equal(gz.view(np.int32), c.g_zq.view(np.int32))
    gz, gw = check_bwd(c, g_zq=False)
    assert not gw.any() and not gz.any()


@gpu
@pytest.mark.parametrize("kind,B", [("range_within", 2), ("range_across", 4)])
def test_vq_backward_dynamic_range_within_and_across_ranges(kind, B):
    """(d) one |d| ~ 2^20 next to a row whose members are all below 2^-12: inside one range the bound lets that row collapse;
    in ANOTHER range the row must be accurate to its own range's quantum (a kernel with one global maximum would not be)"""
    c = Case(kind, B, 32, 32, 64)
    _check_range_case(c, bwd_reference(c.z, c.cb, c.idx, None, 3.0, True)[0])
    check_bwd(c)


@gpu
def test_vq_backward_a_range_of_subnormal_differences_counts_as_zero():
    """two ranges: ordinary differences in the first, only subnormal ones (on rows of their own) in the second -- those rows get
    an exactly zero gradient, as documented; g_z keeps its subnormal products"""
    c = Case("subnormal_range", 4, 32, 32, 64)
    gz, gw = check_bwd(c, g_zq=False)
    assert gw[:32].all() and not gw[32:].any()
    check_bwd(c)


@gpu
@pytest.mark.parametrize("g_loss", [0.0, 3.0, None])
def test_vq_backward_optional_arguments(g_loss):
    """(e) g_loss 0 / 3 / absent, g_zq absent, one gradient only in each direction"""
    c = Case("randn", 3, 683, 1, 1024)
    gz, gw = check_bwd(c, g_loss=g_loss)
    gz2, gw2 = check_bwd(c, g_loss=g_loss, g_zq=False)
    if g_loss in (0.0, None):
        assert not gw.any() and not gz2.any() and np.array_equal(gz, c.g_zq)
    only_gz, none = run_bwd(c, g_loss, want_gw=False)
    assert none is None and np.array_equal(only_gz.view(np.int32), gz.view(np.int32))
    none, only_gw = run_bwd(c, g_loss, want_gz=False)
    assert none is None and np.array_equal(only_gw.view(np.int32), gw.view(np.int32))


@gpu
def test_vq_backward_empty_batch_gives_a_zero_codebook_gradient():
    """(f)"""
    c = Case("randn", 0, 8, 8, 1024)
    gz, gw = run_bwd(c)
    assert gz.shape == (0, 4, 8, 8) and gw.shape == (1024, 4) and not gw.any()


@gpu
def test_vq_backward_is_identical_from_run_to_run_at_the_capped_grid():
    """(g)"""
    c = Case("randn", *BIG, 1024, seed=1)
    first = run_bwd(c)
    for _ in range(2):
        again = run_bwd(c)
        assert np.array_equal(first[0].view(np.int32), again[0].view(np.int32)) and np.array_equal(first[1].view(np.int32), again[1].view(np.int32))


# ---------------------------------------------------------------------------- an infinite loss gradient (include/cgic_hip.h)
@gpu
def test_vq_backward_with_an_infinite_loss_gradient():
    """g_loss = inf: both gradients are non-finite exactly where the CPU expression is -- inf * 0 is NaN (vectors that sit on
    their code, rows that no vector uses), inf * d an infinity"""
    c = Case("randn", 4, 32, 32, 64)
    c.idx[c.idx == 7] = 8                                                 # an unused row: its sum is 0
    zf = flat(c.z)
    zf[::5] = c.cb[c.idx[::5]]                                            # d = 0 in every fifth vector
    z = unflat(zf, c.B, c.h, c.w)
    d, ce, want_gz, want_gw = bwd_reference(z, c.cb, c.idx, c.g_zq, np.inf, True)
    assert np.isnan(want_gz).sum() == 4 * len(zf[::5]) and np.isinf(want_gz).sum() == want_gz.size - 4 * len(zf[::5])
    assert np.isnan(want_gw[7]).all() and not np.isfinite(want_gw).any()
    gz, gw = run_bwd(c, g_loss=np.inf, z=z)
    assert_same_bits(gz, want_gz)
    assert np.array_equal(np.isfinite(gw), np.isfinite(want_gw)) and np.isnan(gw[7]).all()
    assert np.array_equal(np.isnan(gw), np.isnan(want_gw)) and np.array_equal(gw[~np.isnan(gw)], want_gw[~np.isnan(gw)].astype(F32))


# ---------------------------------------------------------------------------- merge, pools, blends (CPU torch = the reference)
def up(t, k):
    return torch.nn.Upsample(scale_factor=k, mode="nearest")(t) if t.numel() else t.repeat_interleave(k, -2).repeat_interleave(k, -1)


# the router's seven modes = the non-empty subsets of {coarse, medium, fine} that a batch is routed to; "overlap": independent
# 0/1 masks (no router makes them; the kernels are products and sums and must follow the expression there too)
MODES = ["cmf", "cm", "cf", "mf", "c", "m", "f", "overlap"]


def make_masks(mode, B, h, w, seed=0):
    """exclusive int32 masks [B,1,h/4,w/4], [B,1,h/2,w/2], [B,1,h,w] that route every fine position to exactly one grain"""
    rng = np.random.default_rng([seed, B, h, w, MODES.index(mode)])
    if mode == "overlap":
        return [torch.from_numpy(rng.integers(0, 2, (B, 1, h // s, w // s)).astype(np.int32)) for s in (4, 2, 1)]
    rep = lambda a, k: a.repeat(k, -2).repeat(k, -1)
    mc = (rng.random((B, 1, h // 4, w // 4)) < 0.4) if "c" in mode and len(mode) > 1 else np.full((B, 1, h // 4, w // 4), mode == "c")
    mm = (rng.random((B, 1, h // 2, w // 2)) < 0.5) if "m" in mode and "f" in mode else np.full((B, 1, h // 2, w // 2), "m" in mode)
    mm &= ~rep(mc, 2)
    mf = ~rep(mc, 4) & ~rep(mm, 2)
    if "f" not in mode and "m" not in mode:
        assert not mf.any()
    assert (rep(mc, 4).astype(int) + rep(mm, 2) + mf == 1).all()
    return [torch.from_numpy(np.ascontiguousarray(m).astype(np.int32)) for m in (mc, mm, mf)]


def ref_merge(hc, hm, hf, mk):
    return up(hc, 4) * up(mk[0].float(), 4) + up(hm, 2) * up(mk[1].float(), 2) + hf * mk[2]               # vqvae_blocks.py:364-366


def ref_blend_medium(hin, own, mk):
    return hin * up(mk[0].float(), 2) + own * mk[1]                                                     # decoder.py:373-374


def ref_blend_fine(hin, own, mk):
    return hin * up(mk[0].float(), 4) + hin * up(mk[1].float(), 2) + own * mk[2]                          # decoder.py:376-378


def same_bits(got, want):
    assert got.dtype == torch.float32 and want.dtype == torch.float32
    assert_same_bits(got.cpu().numpy(), want.numpy())


def cuda(ts):
    return [t.cuda() for t in ts]


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def check_streams(B, C, h, w, mode, seed=0, plant=None):
    """grain merge + fine blend on the fine grid [B,C,h,w], medium blend on [B,C,h/2,w/2], both pools, against the CPU"""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * B + C + h + w)
    mk = make_masks(mode, B, h, w, seed)
    hc, hm, hf, own = randn(gen, B, C, h // 4, w // 4), randn(gen, B, C, h // 2, w // 2), randn(gen, B, C, h, w), randn(gen, B, C, h, w)
    own_m = randn(gen, B, C, h // 2, w // 2)
    if plant is not None:
        plant(mk, hc, hm, hf, own, own_m)
    dmk = cuda(mk)
    same_bits(cg.grain_merge(*cuda((hc, hm, hf)), dmk), ref_merge(hc, hm, hf, mk))
    same_bits(cg.decoder_blend_fine(*cuda((hf, own)), dmk), ref_blend_fine(hf, own, mk))
    same_bits(cg.decoder_blend_medium(*cuda((hm, own_m)), dmk[:2]), ref_blend_medium(hm, own_m, mk[:2]))
    buf = hf.cuda()
    assert cg.decoder_blend_fine(buf, own.cuda(), dmk, out=buf) is buf                                   # the raw, in-place path
    same_bits(buf, ref_blend_fine(hf, own, mk))
    buf = hm.cuda()
    assert cg.decoder_blend_medium(buf, own_m.cuda(), dmk[:2], out=buf) is buf
    same_bits(buf, ref_blend_medium(hm, own_m, mk[:2]))
    for k in (2, 4):
        same_bits(cg.avg_pool(hf.cuda(), k), torch.nn.functional.avg_pool2d(hf, k, k, 0) if B else hf.new_empty(0, C, h // k, w // k))
    return mk, hc, hm, hf, own, own_m


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,h,w", [(1, 1, 4, 4), (2, 3, 4, 8), (1, 2, 8, 4), (2, 1, 12, 20), (0, 3, 8, 8)])
def test_streams_small_shapes_in_every_mode(B, C, h, w, mode):
    """medium grids 2 / 4 / 2 / 10 wide: widths 2 and 10 take unit 2 (1 and 5 threads per row)"""
    check_streams(B, C, h, w, mode)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,hh,ww", [(2, 2, 4, 2), (1, 3, 6, 6), (2, 1, 2, 6)])
def test_medium_blend_on_grids_2_and_6_wide(B, C, hh, ww, mode):
    """unit 2 with one and three threads per row"""
    gen = torch.Generator().manual_seed(hh * ww)
    mk = make_masks(mode, B, 2 * hh, 2 * ww)[:2]
    hin, own = randn(gen, B, C, hh, ww), randn(gen, B, C, hh, ww)
    same_bits(cg.decoder_blend_medium(hin.cuda(), own.cuda(), cuda(mk)), ref_blend_medium(hin, own, mk))


# past the grid caps (8192 workgroups for the merge, 16384 for pools and blends): odd quarter / half widths, so that the
# grid stride wraps in the middle of a row
@gpu
def test_grain_merge_beyond_its_grid_cap():
    B, C, h, w = 3, 96, 64, 508
    assert B * C * h * (w // 4) > 8192 * 256 and (w // 4) % 2 == 1
    gen = torch.Generator().manual_seed(1)
    mk = make_masks("cmf", B, h, w)
    hc, hm, hf = randn(gen, B, C, h // 4, w // 4), randn(gen, B, C, h // 2, w // 2), randn(gen, B, C, h, w)
    same_bits(cg.grain_merge(*cuda((hc, hm, hf)), cuda(mk)), ref_merge(hc, hm, hf, mk))


@gpu
@pytest.mark.parametrize("which,w", [("fine", 508), ("medium", 508), ("medium", 510)])
def test_blends_beyond_the_grid_cap(which, w):
    """508: unit 4 with 127 threads per row; 510: unit 2 with 255"""
    B, C, h = 2, 130, 128
    assert B * C * h * (w // 4) > 16384 * 256
    gen = torch.Generator().manual_seed(w)
    hin, own = randn(gen, B, C, h, w), randn(gen, B, C, h, w)
    if which == "fine":
        mk = make_masks("cmf", B, h, w)
        same_bits(cg.decoder_blend_fine(hin.cuda(), own.cuda(), cuda(mk)), ref_blend_fine(hin, own, mk))
    else:
        mk = make_masks("cmf", B, 2 * h, 2 * w)[:2]
        same_bits(cg.decoder_blend_medium(hin.cuda(), own.cuda(), cuda(mk)), ref_blend_medium(hin, own, mk))


@gpu
@pytest.mark.parametrize("k,H", [(2, 256), (4, 512)])
def test_avg_pool_beyond_the_grid_cap(k, H):
    C = 264
    assert C * (H // k) ** 2 > 16384 * 256
    x = torch.randn(1, C, H, H, generator=torch.Generator().manual_seed(k))
    same_bits(cg.avg_pool(x.cuda(), k), torch.nn.functional.avg_pool2d(x, k, k, 0))


SPECIALS = [np.inf, -np.inf, np.nan, -0.0, float(np.finfo(F32).max), 1e-39, float(np.float32(2.0 ** -149))]


def _plant(t, selected):
    """every special value once where `selected` (broadcast to t) is set and once where it is not"""
    sel = selected.expand_as(t).reshape(-1)
    on, off = torch.nonzero(sel).reshape(-1), torch.nonzero(~sel).reshape(-1)
    assert len(on) >= len(SPECIALS) and len(off) >= len(SPECIALS)
    step_on, step_off = len(on) // len(SPECIALS), len(off) // len(SPECIALS)
    for i, v in enumerate(SPECIALS):
        t.view(-1)[on[i * step_on]] = v
        t.view(-1)[off[i * step_off]] = v


@gpu
@pytest.mark.parametrize("mode", ["cmf", "overlap"])
def test_streams_special_values_in_selected_and_masked_out_positions(mode):
    """products and sums, not selects: an Inf or NaN that the mask zeroes is a NaN in the output like in the reference; -0.0,
    FLT_MAX and subnormals come through with their bits"""
    sub = torch.tensor([2.0 ** -149, 1e-39], dtype=torch.float32)
    assert bool((sub * 1.0 + 0.0 == sub).all()) and bool((sub != 0).all())          # this host does not flush subnormals

    def plant(mk, hc, hm, hf, own, own_m):
        b = [m.bool() for m in mk]
        _plant(hc, b[0])
        _plant(hm, b[1])                                                              # merge: x mask_m; medium blend: x up2(mask_c) (either way both kinds)
        _plant(hf, b[2])                                                              # merge: x mask_f; fine blend: x (up4(mask_c) + up2(mask_m))
        _plant(own, b[2])
        _plant(own_m, b[1])

    mk, hc, hm, hf, own, own_m = check_streams(2, 3, 16, 24, mode, seed=3, plant=plant)
    ref = ref_merge(hc, hm, hf, mk)
    if mode == "cmf":
        assert bool(torch.isnan(ref).any()) and bool((ref.abs() == 2.0 ** -149).any()) and bool(torch.isinf(ref).any())
    zeroed_inf = torch.isinf(hf) & (mk[2] == 0)
    assert bool(zeroed_inf.any()) and bool(torch.isnan(ref[zeroed_inf]).all())          # x * 0 with x = Inf


@gpu
def test_avg_pool_overflow_order_and_subnormal_windows():
    """the window's row-major running sum: FLT_MAX + FLT_MAX - FLT_MAX - FLT_MAX is +Inf in that order (0 in another);
    windows of subnormals average to subnormals"""
    big, tiny = float(np.finfo(F32).max), 2.0 ** -149
    for k in (2, 4):
        x = torch.randn(2, 3, 4 * k, 6 * k, generator=torch.Generator().manual_seed(k))
        win = lambda i, j: x[0, 0, i * k:(i + 1) * k, j * k:(j + 1) * k]
        win(0, 0)[:] = 0.0; win(0, 0)[0, 0] = big; win(0, 0)[0, 1] = big; win(0, 0)[1, 0] = -big; win(0, 0)[1, 1] = -big   # overflows after two terms
        win(0, 1)[:] = 0.0; win(0, 1)[0, 0] = big; win(0, 1)[1, 0] = big; win(0, 1)[0, 1] = -big; win(0, 1)[1, 1] = -big   # row-major: never overflows
        win(1, 0)[:] = tiny
        win(1, 1)[:] = 1e-39
        win(1, 2)[:] = tiny; win(1, 2)[0, 0] = -0.0
        win(2, 0)[:] = -0.0
        win(2, 1)[0, 0] = np.inf; win(2, 1)[-1, -1] = -np.inf
        win(2, 2)[-1, -1] = np.nan
        win(3, 0)[:] = big / 2                                                       # overflows part-way through the sum
        win(3, 1)[:] = -big / 2
        win(3, 2)[:] = big / 32                                                      # a sum near FLT_MAX / 2 that fits
        ref = torch.nn.functional.avg_pool2d(x, k, k, 0)
        assert ref[0, 0, 0, 0] == np.inf and ref[0, 0, 0, 1] == 0 and ref[0, 0, 3, 0] == np.inf and ref[0, 0, 3, 1] == -np.inf
        assert ref[0, 0, 1, 0] == tiny and 0 < ref[0, 0, 1, 1] < 1.2e-38             # the CPU reference kept the subnormals
        assert torch.isnan(ref[0, 0, 2, 1]) and torch.isnan(ref[0, 0, 2, 2]) and torch.isfinite(ref[0, 0, 3, 2])
        same_bits(cg.avg_pool(x.cuda(), k), ref)


# ---------------------------------------------------------------------------- fp32 pointers that allow only a narrower unit
def offset_view(t, elements):
    """t's values in a device tensor whose storage begins `elements` elements before it: a contiguous view at that storage offset"""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device="cuda")
    v = buf[elements:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == elements and v.data_ptr() % 16 == (4 * elements) % 16
    return v


def _f32_call(name, tensors, dims, out):
    """the raw _f32 entry point on exactly these device tensors (no copy, no cast in between)"""
    from control_gic_amd import _lib
    _lib.call(name, *(_lib.ptr(t) for t in tensors), *dims, _lib.ptr(out), _lib.current_stream(out.device))
    return out


@gpu
@pytest.mark.parametrize("elements", [1, 2])
@pytest.mark.parametrize("mode", ["cmf", "overlap"])
def test_fp32_tensors_at_a_storage_offset_take_units_2_and_1(mode, elements):
    """widths that allow 4 floats per thread, one tensor at a time -- each feature, each mask, `out` -- at a pointer aligned to 4
    bytes (offset 1) or 8 bytes (offset 2) only: the 1- or 2-element unit (the plan: tests/test_merge_plan_host.py), the same bits"""
    B, C, h, w = 2, 3, 8, 16
    gen = torch.Generator().manual_seed(10 * elements + MODES.index(mode))
    mk = make_masks(mode, B, h, w)
    hc, hm, hf, own = randn(gen, B, C, h // 4, w // 4), randn(gen, B, C, h // 2, w // 2), randn(gen, B, C, h, w), randn(gen, B, C, h, w)
    own_m = randn(gen, B, C, h // 2, w // 2)
    calls = [      # entry point, inputs, dims, the CPU expression
        ("cgic_grain_merge_f32", (hc, hm, hf, *mk), (B, C, h, w), ref_merge(hc, hm, hf, mk)),
        ("cgic_decoder_blend_fine_f32", (hf, own, *mk), (B, C, h, w), ref_blend_fine(hf, own, mk)),
        ("cgic_decoder_blend_medium_f32", (hm, own_m, *mk[:2]), (B, C, h // 2, w // 2), ref_blend_medium(hm, own_m, mk[:2])),
    ]
    for name, inputs, dims, want in calls:
        for which in range(len(inputs) + 1):                                             # the last one: out
            dev = [offset_view(t, elements) if i == which else t.cuda() for i, t in enumerate(inputs)]
            out = torch.zeros_like(want)
            out = offset_view(out, elements) if which == len(inputs) else out.cuda()
            same_bits(_f32_call(name, dev, dims, out), want)
        if "blend" in name:                                                              # in place: out is h, at the offset with it
            for which in range(len(inputs)):
                dev = [offset_view(t, elements) if i == which else t.cuda() for i, t in enumerate(inputs)]
                same_bits(_f32_call(name, dev, dims, dev[0]), want)
    for k in (2, 4):
        want = torch.nn.functional.avg_pool2d(hf, k, k, 0)
        same_bits(_f32_call("cgic_avgpool_f32", [offset_view(hf, elements)], (B * C, h, w, k), torch.zeros_like(want).cuda()), want)
        if elements == 1:
            same_bits(_f32_call("cgic_avgpool_f32", [hf.cuda()], (B * C, h, w, k), offset_view(torch.zeros_like(want), 1)), want)


@gpu
@pytest.mark.parametrize("k", [2, 4])
def test_fp32_avg_pool_keeps_the_sign_of_a_negative_average_that_underflows(k):
    """a window of zeros and one -2^-149: the running sum is -2^-149 and the quotient by k*k rounds to -0.0, which is what the kernel
    stores; the all-zero window next to it gives +0.0.  ATen's CPU kernel returns +0 in the first place (it adds the average onto a
    zeroed output element, and 0 + -0 is +0); the kernel's value is kept on purpose, as it has been since the fp32 pool was
    written (the half pools store +0: tests/test_merge_half.py)"""
    x = torch.zeros(1, 1, 2 * k, 2 * k)
    x[0, 0, 1, 1] = -2.0 ** -149
    want = np.zeros((1, 1, 2, 2), F32)
    with np.errstate(under="ignore"):
        want[0, 0, 0, 0] = np.float32(-2.0 ** -149) / np.float32(k * k)
    assert want.view(np.uint32).reshape(-1).tolist() == [0x80000000, 0, 0, 0]
    got = cg.avg_pool(x.cuda(), k).cpu().numpy()
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------- autograd at the edges (fp64 CPU autograd = the reference)
def _leaf(t, dev=None):
    return (t.cuda() if dev else t.double()).requires_grad_()


def _window_tol(g, k):
    """a k x k window sum in fp32 costs at most (k^2 - 1) * 2^-24 * sum |g| over the window; the x16, x4, / k^2 scalings are exact"""
    return (k * k - 1) * 2.0 ** -24 * torch.nn.functional.avg_pool2d(g.double().abs(), k, k, 0) * (k * k)


@gpu
@pytest.mark.parametrize("squeezed", [True, False])
def test_merge_gradients_with_batch_equal_to_channels_and_a_permuted_gradient(squeezed):
    """B == C == 3 with [B,h,w] masks (they must broadcast over the CHANNELS, not line up with them) and an incoming
    gradient that is a permuted view: window-sum gradients within the derived bound, elementwise ones bit-exact"""
    B = C = 3
    h, w = 8, 12
    gen = torch.Generator().manual_seed(31)
    mk = make_masks("cmf", B, h, w, seed=2)
    assert not torch.equal(mk[2][0], mk[2][1])                                       # the images differ: a mix-up of the axes shows
    ts = [randn(gen, B, C, h // 4, w // 4), randn(gen, B, C, h // 2, w // 2), randn(gen, B, C, h, w)]
    wgt = randn(gen, B, C, w, h)                                                     # multiplies out.permute(0, 1, 3, 2)
    g_out = wgt.permute(0, 1, 3, 2)
    a, b = [_leaf(t, "cuda") for t in ts], [_leaf(t) for t in ts]
    dmk = [m.cuda().reshape(B, *m.shape[2:]) if squeezed else m.cuda() for m in mk]
    out = cg.grain_merge(a[0], a[1], a[2], dmk)
    (out.permute(0, 1, 3, 2) * wgt.cuda()).sum().backward()
    ref = ref_merge(b[0], b[1], b[2], [m.double() for m in mk])
    (ref.permute(0, 1, 3, 2) * wgt.double()).sum().backward()
    same_bits(out.detach(), ref_merge(*ts, mk))
    assert torch.equal(a[2].grad.cpu().double(), b[2].grad)                          # g * mask_f: exact
    for i, k in ((0, 4), (1, 2)):
        err = (a[i].grad.cpu().double() - b[i].grad).abs()
        assert bool((err <= _window_tol(g_out, k) * mk[i].double()).all()), float(err.max())
        assert bool((a[i].grad.cpu()[(mk[i] == 0).expand_as(ts[i])] == 0).all())


@gpu
def test_pool_and_blend_gradients_with_batch_equal_to_channels_and_a_permuted_gradient():
    B = C = 3
    h, w = 8, 12
    gen = torch.Generator().manual_seed(37)
    mk = make_masks("overlap", B, h, w, seed=4)                                      # the fine blend's weight reaches 2
    dsq = [m.cuda().reshape(B, *m.shape[2:]) for m in mk]
    for k in (2, 4):
        x, wk = randn(gen, B, C, h, w), randn(gen, B, C, w // k, h // k)
        a, b = _leaf(x, "cuda"), _leaf(x)
        (cg.avg_pool(a, k).permute(0, 1, 3, 2) * wk.cuda()).sum().backward()
        (torch.nn.functional.avg_pool2d(b, k, k, 0).permute(0, 1, 3, 2) * wk.double()).sum().backward()
        assert torch.equal(a.grad.cpu().double(), b.grad)                            # g / k^2, repeated: exact
    for fine in (False, True):
        s = 1 if fine else 2
        ts = [randn(gen, B, C, h // s, w // s), randn(gen, B, C, h // s, w // s)]
        wgt = randn(gen, B, C, w // s, h // s)
        a, b = [_leaf(t, "cuda") for t in ts], [_leaf(t) for t in ts]
        m64 = [m.double() for m in mk]
        if fine:
            out, ref = cg.decoder_blend_fine(a[0], a[1], dsq), ref_blend_fine(b[0], b[1], m64)
        else:
            out, ref = cg.decoder_blend_medium(a[0], a[1], dsq[:2]), ref_blend_medium(b[0], b[1], m64[:2])
        (out.permute(0, 1, 3, 2) * wgt.cuda()).sum().backward()
        (ref.permute(0, 1, 3, 2) * wgt.double()).sum().backward()
        assert torch.equal(a[0].grad.cpu().double(), b[0].grad) and torch.equal(a[1].grad.cpu().double(), b[1].grad)


# ---------------------------------------------------------------------------- argument holes: every case raises before any launch
def _merge_args(B=2, C=3, h=8, w=8):
    z = lambda *s: torch.zeros(*s, device="cuda")
    mk = [torch.ones(B, 1, h // s, w // s, dtype=torch.int32, device="cuda") for s in (4, 2, 1)]
    return z(B, C, h // 4, w // 4), z(B, C, h // 2, w // 2), z(B, C, h, w), mk


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bool, torch.int64])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_masks_that_are_not_int32_are_refused(dtype, which):
    """a float mask (the reference's own mask.float()) would be read as the integer 1065353216"""
    hc, hm, hf, mk = _merge_args()
    mk[which] = mk[which].to(dtype)
    msg = "masks must be int32 like the router's"
    with pytest.raises(TypeError, match=msg):
        torch.ops.cgic.grain_merge(hc, hm, hf, *mk)
    with pytest.raises(TypeError, match=msg):
        torch.ops.cgic.decoder_blend_fine(hf, hf, *mk)
    with pytest.raises(TypeError, match=msg):
        cg.decoder_blend_fine(hf, hf, mk, out=torch.empty_like(hf))
    if which < 2:
        with pytest.raises(TypeError, match=msg):
            torch.ops.cgic.decoder_blend_medium(hm, hm, mk[0], mk[1])
        with pytest.raises(TypeError, match=msg):
            cg.decoder_blend_medium(hm, hm, mk[:2], out=torch.empty_like(hm))


@gpu
@pytest.mark.parametrize("which", [0, 1, 2])
def test_grain_merge_refuses_a_mask_of_the_wrong_size(which):
    hc, hm, hf, mk = _merge_args()
    mk[which] = mk[which][:1]                                                        # one image short: would be read out of bounds
    with pytest.raises(ValueError, match="grain_merge: masks"):
        torch.ops.cgic.grain_merge(hc, hm, hf, *mk)
    with pytest.raises(ValueError, match="grain_merge: masks"):
        cg.grain_merge(hc, hm, hf, mk)


@gpu
def test_vq_backward_checks_types_and_sizes():
    z = torch.zeros(2, 4, 4, 4, device="cuda")
    cb = torch.zeros(16, 4, device="cuda")
    idx = torch.zeros(32, dtype=torch.int64, device="cuda")
    gl = torch.ones((), device="cuda")
    for bad in ((z.half(), cb, idx), (z.double(), cb, idx), (z, cb.double(), idx), (z, cb.half(), idx), (z, cb, idx.int()), (z, cb, idx.float())):
        with pytest.raises(TypeError, match="vq_backward"):
            vq_backward(*bad, z, gl, BETA, True)
    for bad in ((z, cb, idx[:31]), (z, cb, torch.cat([idx, idx])), (z, cb[:, :3].contiguous(), idx), (z, cb.reshape(-1), idx),
                (z[:, :3].contiguous(), cb[:, :3].contiguous(), idx)):
        with pytest.raises(ValueError, match="vq_backward"):
            vq_backward(*bad, None, gl, BETA, True)
    for g_zq, g_loss in ((z.half(), gl), (z.double(), gl), (z, gl.double()), (z, gl.half())):
        with pytest.raises(TypeError, match="vq_backward"):
            vq_backward(z, cb, idx, g_zq, g_loss, BETA, True)
    for g_zq, g_loss in ((z[:1], gl), (z, torch.ones(2, device="cuda"))):
        with pytest.raises(ValueError, match="vq_backward"):
            vq_backward(z, cb, idx, g_zq, g_loss, BETA, True)
    with pytest.raises(TypeError, match="vq_backward"):
        torch.ops.cgic.vq_backward(z, cb, idx.int(), z, gl, BETA, True)
    gz, gw = vq_backward(z, cb, idx, z, gl, BETA, True)                              # the good call next to them goes through
    assert not gz.any() and not gw.any()


@gpu
@pytest.mark.parametrize("k,H,W", [(2, 7, 8), (2, 8, 7), (4, 8, 10), (4, 6, 8), (3, 9, 9)])
def test_avg_pool_refuses_shapes_the_window_does_not_divide(k, H, W):
    """(the reference's AvgPool2d would drop the remainder; the decoder never has one)"""
    with pytest.raises(cg.CgicError, match="avgpool"):
        cg.avg_pool(torch.zeros(1, 2, H, W, device="cuda"), k)
