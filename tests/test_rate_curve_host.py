"""CPU: the host side of the rate curve -- the router's rank arithmetic as the library exports it (cgic_router_ranks), the
ratio that reaches a rank (ratio_for_rank), choose on a RateCurve, and the argument validation of cgic_rate_curve (which runs
before anything touches a device)."""
import ctypes

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib
from oracle import cgic_oracle as orc


def _ranks(c, m, n16):
    kc, km = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _lib.lib().cgic_router_ranks(c, m, n16, ctypes.byref(kc), ctypes.byref(km))
    return rc, kc.value, km.value


def test_router_ranks_are_python_round_of_the_products():
    ratios = [0.0, 1e-9, 0.05, 0.1, 0.125, 0.2, 0.25, 0.3, 1 / 3, 0.375, 0.5, 0.625, 0.7, 0.75, 0.9, 1.0]
    seen = set()
    for n16 in (1, 2, 4, 6, 24, 100, 256, 1000, 2304, 3072):
        n8 = 4 * n16
        for c in ratios:
            for m in ratios:
                mode = orc.router_mode(c, m)
                # RouterTriple.py:23,30,42,54,65: the ranks each mode takes, 0 where it takes none
                kc = round(n16 * c) if mode in (0, 2, 3) else 0
                km = round((4 * n16) * c + n8 * m) if mode == 0 else round(n8 * m) if mode == 1 else 0
                rc, gc, gm = _ranks(c, m, n16)
                if kc > n16 or km > n8:
                    assert rc == _lib.ERR_INVALID, (c, m, n16)
                    assert b"k out of range" in _lib.lib().cgic_last_error()
                    seen.add("invalid")
                else:
                    assert (rc, gc, gm) == (_lib.OK, kc, km), (c, m, n16, mode)
                    seen.add(mode)
    assert seen == {0, 1, 2, 3, 4, 5, 6, "invalid"}
    # halves round to even, like Python: 0.125 * 4 = 0.5 -> 0, 0.375 * 4 = 1.5 -> 2, 0.625 * 4 = 2.5 -> 2
    assert [_ranks(0.0, m, 1)[2] for m in (0.125, 0.375, 0.625)] == [0, 2, 2]
    assert cg.router_ranks(0.1, 0.4, 256) == (26, round(1024 * 0.1 + 1024 * 0.4))
    with pytest.raises(cg.CgicError):
        cg.router_ranks(0.5, 0.7, 256)
    assert _lib.lib().cgic_router_ranks(0.1, 0.4, 0, None, None) == _lib.ERR_INVALID
    assert _lib.lib().cgic_router_ranks(0.1, 0.4, 16, None, None) == _lib.OK        # (outputs are optional)


@pytest.mark.parametrize("n16", [256, 2304])
@pytest.mark.parametrize("c", [0.0, 0.05, 0.1, 0.3])
def test_ratio_for_rank(n16, c):
    n8 = 4 * n16
    want_mode = 0 if c > 0 else 1
    got = []
    for K in range(n8 + 1):
        m = cg.ratio_for_rank(K, n16, c)
        if m is None:
            continue
        assert 0.0 < m <= 1.0
        assert orc.router_mode(c, m) == want_mode, (K, m)
        k = round((4 * n16) * c + n8 * m) if want_mode == 0 else round(n8 * m)
        assert k == K, (K, m, k)
        got.append(K)
    # one contiguous run: from the first rank a positive medium ratio gives (round(4 n16 c)) to the top
    assert got == list(range(got[0], got[-1] + 1))
    assert got[0] == round((4 * n16) * c) and got[-1] == n8
    assert len(got) >= n8 - round((4 * n16) * c)
    assert [k for k, _ in cg.rate.reachable_ranks(n16, c)] == got
    if c > 0:
        assert cg.ratio_for_rank(got[0] - 1, n16, c) is None


def _curve(bpp_rows, ranks, c=0.1):
    """a RateCurve from per-image bpp values [B][n8 + 1] of 256x256 images (bytes = bpp * 256^2 / 8)"""
    bpp = np.asarray(bpp_rows, np.float64)
    nb = np.zeros(bpp.shape + (5,), np.int32)
    nb[..., 2] = np.round(bpp * 256 * 256 / 8).astype(np.int32)
    return cg.RateCurve(torch.from_numpy(nb), c, 256 * 256, ranks=ranks)


def test_choose_on_a_non_monotone_curve():
    #      K:    0     1     2     3     4     5     6     7     8
    img0 = [0.90, 0.80, 0.50, 0.60, 0.60, 0.30, 0.40, 0.20, 0.10]
    img1 = [0.90, 0.80, 0.70, 0.40, 0.40, 0.50, 0.20, 0.40, 0.10]
    ranks = [(k, 0.1 * k) for k in range(2, 9)]          # ranks 0 and 1: no ratio reaches them
    t = _curve([img0, img1], ranks)
    assert t.bytes.shape == (2, 9) and t.batch_bpp.shape == (9,) and t.ranks == list(range(2, 9))
    assert abs(t.batch_bpp[2].item() - 0.6) < 1e-3
    # batch curve over K = 2..8: 0.6 0.5 0.5 0.4 0.3 0.3 0.1 -- the largest <= target; ties -> the smaller medium ratio
    assert cg.choose(t, 0.55) == (3, True)
    assert cg.choose(t, 0.35) == (6, True)
    assert cg.choose(t, 0.45) == (5, True)
    assert cg.choose(t, 10.0) == (2, True)               # 0.9 / 0.8 at ranks 0, 1 are not reachable
    assert cg.choose(t, 0.05) == (8, False)
    assert t.ratio(5) == (0.1, 0.5)
    # per image: img0 is not monotone (0.5 at K = 2, 0.6 at K = 3, 4; 0.3 at 5, 0.4 at 6): a bisection would miss these
    k, f = cg.choose(t, 0.45, per="image")
    assert k.tolist() == [6, 3] and f.tolist() == [True, True]
    k, f = cg.choose(t, 0.65, per="image")
    assert k.tolist() == [3, 5] and f.tolist() == [True, True]
    k, f = cg.choose(t, 0.05, per="image")
    assert k.tolist() == [8, 8] and f.tolist() == [False, False]
    with pytest.raises(ValueError):
        cg.choose(t, 1.0, per="pixel")
    with pytest.raises(ValueError):
        cg.choose(_curve([img0], []), 1.0)
    bad = np.zeros((1, 9, 5), np.int32)
    bad[0, 4, 1] = -11
    with pytest.raises(KeyError):
        cg.RateCurve(torch.from_numpy(bad), 0.1, 256 * 256, ranks=ranks)


def _call(coarse=0.1, B=2, h16=4, w16=4, ptrs=None, nbytes=0x1000, ws=0x2000, table=True):
    coder = cg.HuffmanCoding({str(i): torch.tensor([float(1 + i)]) for i in range(16)})
    p = [0x10000] * 5 if ptrs is None else ptrs
    return _lib.lib().cgic_rate_curve(coder.table.handle if table else None, p[0], p[1], p[2], p[3], p[4], B, h16, w16, coarse,
                                      nbytes, ws, None)


def test_argument_validation_before_any_launch():
    for i in range(5):
        p = [0x10000] * 5
        p[i] = None
        assert _call(ptrs=p) == _lib.ERR_INVALID
    assert _call(nbytes=None) == _lib.ERR_INVALID
    assert _call(table=False) == _lib.ERR_INVALID
    assert b"NULL" in _lib.lib().cgic_last_error()
    assert _call(ws=None) == _lib.ERR_INVALID                       # workspace required
    assert b"workspace" in _lib.lib().cgic_last_error()
    assert _call(ws=0x2004) == _lib.ERR_INVALID                     # ... and 16-byte aligned
    assert _call(coarse=-0.1) == _lib.ERR_INVALID
    assert _call(coarse=1.5) == _lib.ERR_INVALID
    assert _call(coarse=float("nan")) == _lib.ERR_INVALID
    assert _call(h16=0) == _lib.ERR_INVALID
    assert _call(B=-1) == _lib.ERR_INVALID
    # an image whose words do not fit one workgroup's LDS: 12288 8x8 patches at most (768x768 has 9216)
    assert _call(h16=64, w16=64) == _lib.ERR_UNSUPPORTED
    assert b"LDS" in _lib.lib().cgic_last_error()
    assert _call(h16=1 << 40, w16=1 << 40) == _lib.ERR_UNSUPPORTED
    assert _call(B=70000) == _lib.ERR_UNSUPPORTED
    assert _call(B=0) == _lib.OK                                    # an empty batch launches nothing


def test_workspace_bytes():
    l = _lib.lib()
    n = l.cgic_rate_curve_workspace_bytes(64, 16, 16)
    assert n >= 64 * 16 and n % 256 == 0
    assert l.cgic_rate_curve_workspace_bytes(0, 16, 16) == 0
    assert l.cgic_rate_curve_workspace_bytes(1, 0, 16) == 0
