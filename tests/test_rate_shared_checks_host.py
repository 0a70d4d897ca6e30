"""CPU: the checks the three curve entry points share (cgic_rate_curve, cgic_rate_curve_tiles, cgic_route_to_budget: one set of
host helpers in cgic_rate_curve.hip) -- every shared failure gives each entry point the same code, and a message that starts with
that entry point's own name.  All of it runs before anything touches a device: the pointers are fake, so no call here is one
that would pass the checks."""
import ctypes
import functools

import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib

P = 0x10000          # a fake, 16-byte aligned device pointer


@functools.lru_cache(maxsize=None)
def _coder():
    """one coder for all cases, kept alive: the calls take its table's handle"""
    return cg.HuffmanCoding({str(i): torch.tensor([float(1 + i)]) for i in range(16)})


def _table(given):
    return _coder().table.handle if given else None


def _curve(table=True, h16=4, w16=4, coarse=0.1, ws=0x20000):
    return _lib.lib().cgic_rate_curve(_table(table), P, P, P, P, P, 2, h16, w16, coarse, P, ws, None)


def _tiles(table=True, h16=4, w16=4, coarse=0.1, ws=0x20000):
    n16 = h16 * w16
    k_c = round(n16 * coarse) if coarse > 0 else 0                     # (NaN: 0, like the library's expression)
    desc = (_lib.RateTile * 1)(_lib.RateTile(h16, w16, k_c, 0, 0, 0, 0, 0, 0, 0, 0))
    count = (ctypes.c_int64 * 5)(n16, 4 * n16, 16 * n16, n16, 4 * n16)
    return _lib.lib().cgic_rate_curve_tiles(_table(table), P, P, P, P, P, count, desc, P, 1, 1, coarse, P, 1, 8, P, None, ws, None)


def _route(table=True, h16=4, w16=4, coarse=0.1, ws=0x20000):
    return _lib.lib().cgic_route_to_budget(_table(table), P, P, P, P, P, 2, h16, w16, coarse, P, 10, P, P, P, P, P, P, ws, None)


FAILURES = {
    "table missing": (dict(table=False), "ERR_INVALID", b"NULL"),
    "64x64 coarse patches": (dict(h16=64, w16=64), "ERR_UNSUPPORTED", b"LDS"),
    "NaN coarse ratio": (dict(coarse=float("nan")), "ERR_INVALID", b"coarse ratio"),
    "workspace missing": (dict(ws=None), "ERR_INVALID", b"workspace"),
    "workspace misaligned": (dict(ws=0x20004), "ERR_INVALID", b"aligned"),
}


@pytest.mark.parametrize("failure", list(FAILURES))
@pytest.mark.parametrize("name, call", [("rate_curve", _curve), ("rate_curve_tiles", _tiles), ("route_to_budget", _route)])
def test_shared_failures_keep_their_code_and_the_entry_points_name(name, call, failure):
    kw, code, word = FAILURES[failure]
    assert call(**kw) == getattr(_lib, code)
    msg = _lib.lib().cgic_last_error()
    assert msg.startswith(name.encode() + b":"), msg
    assert word in msg, msg
