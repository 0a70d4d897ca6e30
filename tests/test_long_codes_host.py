"""CPU: code tables whose longest code has 14 to 65 bits.  tests/golden/long_codes.npz holds what the REAL reference coder makes of
the ladder tables of tests/long_codes_ref.py (tests/golden/make_golden_longcodes.py): lengths, code words of one, two and three
32-bit words, and the bytes of short streams.  The oracle's table, encoder and decoder are pinned to it here, and so is the table
the native library builds (cgic_table_create runs on the host) -- what tests/test_long_codes.py then demands of the GPU coders."""
import numpy as np
import pytest

import long_codes_ref as lc

TABLES = [pytest.param(K, L, id=f"k{K}-l{L}") for K, L in lc.FIXTURE_TABLES]
STREAMS = ("n0", "n1", "n2", "n65") + lc.CONTENT


@pytest.mark.parametrize("K", [96, 1024, 2560])
def test_ladder_table_reaches_every_target(orc, K):
    """the helper's own promise, held with the oracle's table builder instead of the helper's: a ladder exists for every longest
    code asked for, and the counts are exact as the floats the Python layer passes"""
    for max_len in (14, 31, 32, 33, 48, 63, 64, 65):
        counts = lc.ladder_table(K, max_len)
        assert counts.dtype == np.int64 and len(counts) == K and int(counts.min()) == 1
        assert np.array_equal(counts.astype(np.float64).astype(np.int64), counts) and int(counts.sum()) < 2 ** 53
        t = orc.HuffmanTable(counts)
        assert t.maxlen == max_len and np.array_equal(t.len, lc.huffman_lengths(counts))
        D = int((counts > 1).sum())
        assert sorted(t.len[counts > 1].tolist()) == list(range(1, D + 1))      # the rungs: one code of every length 1 .. D


def test_fixture_is_the_helpers_tables(golden):
    g = golden("long_codes")
    assert [tuple(r) for r in g["tables"].tolist()] == list(lc.FIXTURE_TABLES)
    for K, L in lc.FIXTURE_TABLES:
        key = f"k{K}_l{L}"
        assert np.array_equal(g[key + "_counts"], lc.ladder_table(K, L))
        lens = g[key + "_len"].astype(np.int32)
        assert int(lens.max()) == L and g[key + "_code"].shape == (K, (L + 31) // 32)
        for name, sym in lc.fixture_streams(lens):
            assert np.array_equal(g[f"{key}_{name}_sym"].astype(np.int64), sym), (key, name)
    # the lengths the GPU tests must reach exist in the tables that are there to supply them
    assert {32, 33} <= set(g["k1024_l33_len"].tolist()) and 32 in g["k1024_l32_len"] and lc.LUT_BITS + 1 in g["k1024_l14_len"]


@pytest.mark.parametrize("K,L", TABLES)
def test_oracle_table_and_streams_match_the_reference(orc, golden, K, L):
    g, key = golden("long_codes"), f"k{K}_l{L}"
    t = orc.HuffmanTable(g[key + "_counts"])
    assert t.maxlen == L and t.words == (L + 31) // 32
    assert np.array_equal(t.len, g[key + "_len"].astype(np.int32)) and np.array_equal(t.code, g[key + "_code"])
    if t.words > 1:       # the fixture really holds bits beyond the first word: a code table cut to one word would differ
        assert np.any(g[key + "_code"][:, 1:] != 0)
    for name in STREAMS:
        sym = g[f"{key}_{name}_sym"].astype(np.int64)
        data = g[f"{key}_{name}_bytes"].tobytes()
        assert orc.encode(t, sym) == data, (key, name)
        dec = orc.decode(t, data)
        assert (dec is None and len(sym) == 0) or np.array_equal(dec, sym), (key, name)
        # the reference pads with 1 .. 8 bits behind the codewords and writes the pad count in front
        bits = int(t.len[sym].sum())
        assert len(data) == (0 if len(sym) == 0 else 1 + bits // 8 + 1)


@pytest.mark.parametrize("K,L", TABLES)
def test_native_table_matches_the_reference(golden, K, L):
    """cgic_table_create on the fixture's counts, handed over as the Python layer hands them (floats through a mapping in the
    reference counter's order): the same lengths and code words, cgic_table_max_len, and cgic_table_words 1, 2 or 3"""
    import control_gic_amd as cg
    from control_gic_amd import _lib
    g, key = golden("long_codes"), f"k{K}_l{L}"
    counts = g[key + "_counts"]

    class _V:
        def __init__(self, v): self.v = v
        def item(self): return self.v
    huff = cg.HuffmanCoding({str(s): _V(float(counts[s])) for s in lc.push_order(K)})
    tab = huff.table
    words = {14: 1, 32: 1, 33: 2, 63: 2, 64: 2, 65: 3}[L]
    assert _lib.lib().cgic_table_max_len(tab.handle) == L and _lib.lib().cgic_table_words(tab.handle) == words
    assert _lib.lib().cgic_table_num_symbols(tab.handle) == K and (tab.max_len, tab.words, tab.n) == (L, words, K)
    ln, cd = tab.arrays()
    assert np.array_equal(np.array(ln, np.int32), g[key + "_len"].astype(np.int32))
    assert np.array_equal(np.array(cd, np.uint32).reshape(K, words), g[key + "_code"])
    # the sizes that follow from the longest code: a stream of n symbols, and a slot of a 64x64 grid
    assert _lib.lib().cgic_stream_capacity(tab.handle, 1024) == ((L * 1024 // 8 + 2 + 8) + 15) // 16 * 16
    assert _lib.lib().cgic_compress_slot_bytes(tab.handle, 64, 64) == ((L * 4096 // 8 + 2 + 8) + 15) // 16 * 16


def test_native_table_bounds_the_sum_of_the_counts():
    """counts are bounded through their sum (no node of the tree exceeds it): the 64- and 65-bit ladders, whose largest count lies
    between 2^46 and 2^47, are tables; a sum of 2^62 or a negative count is refused"""
    import ctypes
    from control_gic_amd import _lib
    l = _lib.lib()

    def create(freq):
        f = (ctypes.c_int64 * len(freq))(*freq)
        h = ctypes.c_void_p()
        rc = l.cgic_table_create(f, None, len(freq), ctypes.byref(h))
        if rc == _lib.OK:
            l.cgic_table_destroy(h)
        return rc
    assert 2 ** 46 < int(lc.ladder_table(1024, 64).max()) < 2 ** 47
    assert create([2 ** 61, 2 ** 61 - 1]) == _lib.OK and create([2 ** 53, 1, 1]) == _lib.OK
    assert create([2 ** 61, 2 ** 61]) == _lib.ERR_INVALID and create([2 ** 62, 0]) == _lib.ERR_INVALID
    assert create([1, 2 ** 61, 2 ** 61 - 1]) == _lib.ERR_INVALID and create([3, -1]) == _lib.ERR_INVALID
    assert create([2 ** 46 - 1] * 65536) == _lib.OK                          # what the bound on every count used to allow
