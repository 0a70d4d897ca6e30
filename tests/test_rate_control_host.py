"""CPU: the host side of rate control -- choose / default_candidates, the byte formula behind the rate tables, and the
candidate validation of cgic_rate_table (which runs before anything touches a device)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib
from oracle import cgic_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))


def _table(bpp_rows, cands):
    """a RateTable from per-image bpp values (bytes = bpp * 256^2 / 8)"""
    bpp = np.asarray(bpp_rows, np.float64)
    nb = np.zeros(bpp.shape + (5,), np.int32)
    nb[..., 0] = np.round(bpp * 256 * 256 / 8).astype(np.int32)
    return cg.RateTable(torch.from_numpy(nb), cands, 256 * 256)


def test_default_candidates():
    c = cg.default_candidates(0.1, 16)
    assert len(c) == 16 and all(cc == 0.1 for cc, _ in c)
    assert c[0] == (0.1, 0.0) and c[-1] == (0.1, 1.0 - 0.1)
    assert all(b[1] > a[1] for a, b in zip(c, c[1:]))
    modes = [_lib.lib().cgic_router_mode(*p) for p in c]
    assert modes[0] == 2 and modes[-1] == 3 and set(modes[1:-1]) == {0}
    assert {_lib.lib().cgic_router_mode(*p) for p in cg.default_candidates(0.0, 5)} == {6, 1, 5}
    assert [_lib.lib().cgic_router_mode(*p) for p in cg.default_candidates(1.0, 2)] == [4, 4]
    with pytest.raises(ValueError):
        cg.default_candidates(0.1, 65)
    with pytest.raises(ValueError):
        cg.default_candidates(1.5)


def test_choose_batch_and_image():
    cands = [(0.1, 0.0), (0.1, 0.3), (0.2, 0.3), (0.0, 0.3), (0.1, 0.6)]
    # bytes per image: candidate x image
    t = _table([[0.5, 0.7], [0.3, 0.3], [0.3, 0.3], [0.3, 0.3], [0.1, 0.9]], cands)
    assert t.bytes.shape == (5, 2) and t.bpp.dtype == torch.float64
    assert abs(t.batch_bpp[0].item() - 0.6) < 1e-3
    # largest <= target; ties (0.3 three times) -> smaller coarse, then smaller medium
    assert cg.choose(t, 0.45) == (3, True)
    assert cg.choose(t, 0.6) == (0, True)
    assert cg.choose(t, 0.05) == (3, False)       # none fits: the smallest bpp (0.3, tie -> coarse 0.0)
    c, f = cg.choose(t, 0.35, per="image")
    assert c.tolist() == [3, 3] and f.tolist() == [True, True]
    c, f = cg.choose(t, 0.12, per="image")
    assert c.tolist() == [4, 3] and f.tolist() == [True, False]
    with pytest.raises(ValueError):
        cg.choose(t, 1.0, per="pixel")


def _reference_file_bytes(lens, syms):
    """HuffmanCoding.compress (indices_coding.py:91-124) restated: "" -> 0 bytes, else header byte + bits + 8 - nbits % 8 pad"""
    if len(syms) == 0:
        return 0
    nbits = sum(int(lens[s]) for s in syms)
    return (8 + nbits + (8 - nbits % 8)) // 8


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1023])
def test_byte_formula_against_the_coder(n):
    freq = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)
    htab = orc.HuffmanTable(freq)
    rng = np.random.default_rng(n)
    for trial in range(4):
        syms = rng.integers(0, 1024, n).astype(np.int64)
        if trial == 1 and n:                                           # code lengths summing to a multiple of 8 exactly
            short = int(np.argmin(htab.len))
            syms = np.full(n, short, np.int64)
        data = orc.encode(htab, syms)
        nbits = int(htab.len[syms].sum()) if n else 0
        want = 0 if n == 0 else nbits // 8 + 2
        assert len(data) == want == _reference_file_bytes(htab.len, syms)


def test_golden_sizes_follow_the_formula():
    """the real reference's file sizes (rate.npz) are nbits // 8 + 2 of the symbols the masks select"""
    g = np.load(os.path.join(HERE, "golden", "rate.npz"))
    htab = orc.HuffmanTable(g["counter"])
    for ii in range(len(g["names"])):
        for ci in range(len(g["candidates"])):
            ind = g[f"img{ii}_c{ci}_ind"].astype(np.int64)
            sizes = g[f"img{ii}_c{ci}_sizes"]
            mode = int(g[f"img{ii}_c{ci}_mode"])
            on = orc.mode_streams(mode)
            for s in range(3):
                if not on[s]:
                    assert sizes[s] == 0
            assert sizes[3] == (16 * 16 // 8 + 2 if on[3] else 0) and sizes[4] == (32 * 32 // 8 + 2 if on[4] else 0)
            assert (ind >= 0).all() and (ind < 1024).all()
            assert all(int(sizes[s]) in (0,) or int(sizes[s]) >= 2 for s in range(3))
            nb = [int(htab.len[ind.ravel()].sum())]
            assert nb[0] > 0


def _call(cands, B=2, h16=4, w16=4, nbytes=0x1000, ws=0x2000):
    C = len(cands)
    arr = ctypes.c_double * max(C, 1)
    coder = cg.HuffmanCoding({str(i): torch.tensor([float(1 + i)]) for i in range(16)})
    fake = 0x10000
    return _lib.lib().cgic_rate_table(coder.table.handle, fake, fake, fake, fake, fake, B, h16, w16, C, arr(*[c for c, _ in cands]),
                                      arr(*[m for _, m in cands]), 1, None, nbytes, ws, None)


def test_candidate_validation_before_any_launch():
    # k > n (fine ratio < 0: the medium threshold's k exceeds the patches) -> CGIC_ERR_INVALID, decided on the host
    assert _call([(0.1, 0.8), (0.5, 0.7)]) == _lib.ERR_INVALID
    assert _call([(0.6, 0.6)]) == _lib.ERR_INVALID
    assert b"k out of range" in _lib.lib().cgic_last_error()
    assert _call([(1.2, 0.0)]) == _lib.ERR_INVALID
    assert _call([]) == _lib.ERR_INVALID
    assert _call([(0.1, 0.8)] * 65) == _lib.ERR_INVALID
    assert _call([(0.1, 0.8)], ws=0) == _lib.ERR_INVALID              # workspace required
    with pytest.raises(ValueError):
        cg.rate._check_candidates([(0.1, 0.8)] * 65)


def test_workspace_bytes():
    l = _lib.lib()
    n = l.cgic_rate_table_workspace_bytes(64, 16, 16, 16, 1)
    assert n >= 16 * 64 * 21 * 256 * 4 and n % 256 == 0
    assert l.cgic_rate_table_workspace_bytes(1, 1, 1, 65, 1) == 0
    assert l.cgic_rate_table_workspace_bytes(0, 16, 16, 4, 1) == 0
