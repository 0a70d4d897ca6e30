"""CPU: the host side of the device-side rate pick -- budget_bytes (the byte budget under which the device's integer comparison
picks what `choose` picks on float64 bpp), the new entry points in the prototype table, and the argument validation of
cgic_route_to_budget (which runs before anything touches a device)."""
import math

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib


def _bpp(S, P, B):
    """RateCurve.batch_bpp's expression, as torch evaluates it on the summed bytes"""
    return (torch.tensor([S], dtype=torch.int64).to(torch.float64) * 8 / (P * max(B, 1)))[0].item()


def _check(target, P, B):
    S = cg.budget_bytes(target, P, B)
    assert isinstance(S, int)
    if S < 0:
        assert S == -1 and not _bpp(0, P, B) <= target
        return S
    assert _bpp(S, P, B) <= target < _bpp(S + 1, P, B), (target, P, B, S)
    return S


def test_budget_bytes_random():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        P = int(rng.choice([64 * 64, 64 * 96, 256 * 256, 768 * 768, 1000 * 1504, int(rng.integers(1, 1 << 22))]))
        B = int(rng.choice([1, 2, 3, 7, 64, int(rng.integers(1, 5000))]))
        target = float(rng.choice([rng.uniform(0, 8), rng.uniform(0, 0.01), 10.0 ** rng.uniform(-9, 3)]))
        _check(target, P, B)


def test_budget_bytes_at_exact_boundaries():
    rng = np.random.default_rng(6)
    for _ in range(1000):
        P = int(rng.choice([64 * 64, 64 * 96, 256 * 256, 768 * 768, int(rng.integers(1, 1 << 22))]))
        B = int(rng.choice([1, 2, 3, 64, int(rng.integers(1, 5000))]))
        S = int(rng.choice([0, 1, 2, int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 40))]))
        t = _bpp(S, P, B)
        assert _check(t, P, B) == S                                  # the equality boundary: S itself still fits
        assert _check(math.nextafter(t, math.inf), P, B) == S       # (distinct byte counts are more than one float64 apart)
        below = _check(math.nextafter(t, -math.inf), P, B)
        assert below == S - 1
    assert cg.budget_bytes(-1.0, 4096, 2) == -1 and cg.budget_bytes(0.0, 4096, 2) == 0
    assert cg.budget_bytes(math.inf, 4096, 2) == cg.budget_bytes(1e300, 4096, 2) == 1 << 62
    with pytest.raises(ValueError):
        cg.budget_bytes(math.nan, 4096, 2)
    with pytest.raises(ValueError):
        cg.budget_bytes(1.0, 0, 2)


def test_budget_comparison_is_the_float_comparison():
    """S <= budget_bytes(target) exactly where bpp(S) <= target: what makes the device's pick `choose`'s pick"""
    rng = np.random.default_rng(7)
    P, B = 64 * 96, 3
    for _ in range(200):
        target = float(rng.uniform(0, 4))
        bud = cg.budget_bytes(target, P, B)
        for S in [max(bud - 2, 0), max(bud - 1, 0), bud, bud + 1, bud + 2, int(rng.integers(0, 1 << 16))]:
            assert (S <= bud) == (_bpp(S, P, B) <= target)


def test_new_symbols_in_the_prototype_table():
    assert "cgic_route_to_budget" in _lib.PROTOTYPES and "cgic_route_to_budget_workspace_bytes" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["cgic_route_to_budget"][1]) == 20
    assert _lib.lib().cgic_abi_version() >= 12
    assert {"BppRoute", "budget_bytes", "route_to_bpp"} <= set(cg.__all__)


def test_workspace_bytes():
    l = _lib.lib()
    n = l.cgic_route_to_budget_workspace_bytes(64, 16, 16, 923)
    assert n >= 64 * 16 + 2 * 64 * 923 * 4 and n % 256 == 0
    for bad in ((0, 16, 16, 9), (1, 0, 16, 9), (1, 16, 16, 0), (1, 16, 16, 1026), (1, 64, 64, 9), (70000, 4, 4, 9)):
        assert l.cgic_route_to_budget_workspace_bytes(*bad) == 0
    assert l.cgic_route_to_budget_workspace_bytes(1, 16, 16, 1025) > 0


def _call(coarse=0.1, B=2, h16=4, w16=4, R=10, **kw):
    coder = cg.HuffmanCoding({str(i): torch.tensor([float(1 + i)]) for i in range(16)})
    a = dict(table=coder.table.handle, ind_c=0x10000, ind_m=0x10000, ind_f=0x10000, e16=0x10000, e8=0x10000, ranks=0x10000,
             budget=0x10000, mc=0x10000, mm=0x10000, mf=0x10000, ind=0x10000, choice=0x10000, ws=0x20000)
    a.update(kw)
    return _lib.lib().cgic_route_to_budget(a["table"], a["ind_c"], a["ind_m"], a["ind_f"], a["e16"], a["e8"], B, h16, w16, coarse,
                                           a["ranks"], R, a["budget"], a["mc"], a["mm"], a["mf"], a["ind"], a["choice"], a["ws"], None)


def test_argument_validation_before_any_launch():
    err = _lib.lib().cgic_last_error
    for name in ("table", "ind_c", "ind_m", "ind_f", "e16", "e8", "ranks", "budget", "mc", "mm", "mf", "ind", "choice"):
        assert _call(**{name: None}) == _lib.ERR_INVALID, name
        assert b"NULL" in err()
    assert _call(ws=None) == _lib.ERR_INVALID and b"workspace" in err()
    assert _call(ws=0x20004) == _lib.ERR_INVALID
    for name in ("ind_m", "ind_f", "mm", "mf", "ind", "e8", "budget", "choice"):
        assert _call(**{name: 0x10004}) == _lib.ERR_INVALID and b"aligned" in err()
    # the curve's mode: 0 with a coarse ratio in (0, 1), 1 at 0
    for c in (-0.1, 1.0, 1.5, float("nan")):
        assert _call(coarse=c) == _lib.ERR_INVALID and b"coarse ratio" in err()
    assert _call(R=0) == _lib.ERR_INVALID and b"requested ranks" in err()
    assert _call(R=66) == _lib.ERR_INVALID                          # n8 + 1 = 65 at most
    assert _call(h16=0) == _lib.ERR_INVALID
    assert _call(B=0) == _lib.ERR_INVALID
    assert _call(h16=64, w16=64) == _lib.ERR_UNSUPPORTED and b"LDS" in err()
    assert _call(h16=1 << 40, w16=1 << 40) == _lib.ERR_UNSUPPORTED
    assert _call(B=70000) == _lib.ERR_UNSUPPORTED
