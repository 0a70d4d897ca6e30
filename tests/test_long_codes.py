"""GPU: the entropy coders on code tables whose longest code has 14 to 65 bits, every decoder path.

A table is handled in three ways, by its longest code: up to lut_bits (13) every codeword resolves in the LDS LUT; from 14 to 64
bits a LUT miss continues in the decode trie, per lane, and from 33 bits on a code has two words (the encoder fetches the second
and keeps the table out of LDS); beyond 64 bits (kSplitMaxLen) the serial one-wave decoder runs.  The tables are the ladders of
tests/long_codes_ref.py, pinned to the real reference coder by tests/golden/long_codes.npz (tests/test_long_codes_host.py); the
decoder path of every (batch, grid, table, decoder argument) here is a row of tests/test_decode_plan_host.py, the encoder form a row
of tests/test_coder_plan_host.py.  Every stream is a valid encoder output, and every comparison is equality:

  compressed bytes == the oracle's, image by image (all of them up to 3 images, else the first, the middle and the last);
  decompress gives the merged grid of the encoded indices, the masks, exact codebook rows and status 0,
  the same under decoder="latency", "throughput" and the default.

The masks are the oracle router's on seeded maps, so that a case is known on the CPU: test_no_content_class_is_vacuous reads the
cumulative code lengths of the very streams the GPU cases encode."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import long_codes_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
gpu = pytest.mark.gpu


def _constant(header, name):
    with open(os.path.join(ROOT, "control-gic_amd", "csrc", header)) as f:
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", f.read())
    return int(eval(m.group(1), {"__builtins__": {}}))


class _V:
    def __init__(self, v): self.v = v
    def item(self): return self.v


@functools.lru_cache(maxsize=None)
def _table(K, L):
    """(counts, oracle table) of the ladder of K symbols with a longest code of L bits; the oracle's longest code is asserted"""
    from oracle import cgic_oracle as orc
    orc.build()
    counts = lc.ladder_table(K, L)
    t = orc.HuffmanTable(counts)
    assert t.maxlen == L and t.words == (L + 31) // 32
    return counts, t


@functools.lru_cache(maxsize=None)
def _codec(K, L):
    import control_gic_amd as cg
    counts, _ = _table(K, L)
    cbk = np.random.default_rng(K + L).standard_normal((K, 4)).astype(np.float32)
    codec = cg.GrainCodec({str(s): _V(float(counts[s])) for s in lc.push_order(K)}, torch.from_numpy(cbk).to(DEV))
    assert (codec.huffman.table.max_len, codec.huffman.table.words) == (L, (L + 31) // 32)
    return codec, cbk


def _routes(B, h, w):
    """[(ratio, mode, (mc, mm, mf))]: the oracle router's masks of seeded maps at the three ratio pairs (modes 0, 6 and 3)"""
    from oracle import cgic_oracle as orc
    e16, e8 = lc.entropy_maps(B, h, w, seed=1000 * B + h + w)
    out = []
    for c, m in lc.RATIOS:
        mc, mm, mf, _, mode = orc.router(e16, e8, c, m, per_image=True, want_gate=False)
        out.append(((c, m), mode, (mc, mm, mf)))
    assert [r[1] for r in out] == [0, 6, 3]
    return out


def _streams_of(ind_b, masks, b):
    from oracle import cgic_oracle as orc
    return orc.select(ind_b, masks[0][b, 0], masks[1][b, 0], masks[2][b, 0])


def _run_case(K, L, B, h, w, kinds=lc.CONTENT, ratios=None):
    """one (table, batch, grid): every content class x ratio pair through compress and the three decoder arguments"""
    from oracle import cgic_oracle as orc
    (codec, cbk), (_, htab) = _codec(K, L), _table(K, L)
    cbk_dev = codec.codebook
    grids = lc.grid_contents(htab.len, B, h, w)
    ran = 0
    for (c, m), mode, masks in _routes(B, h, w):
        if ratios is not None and (c, m) not in ratios:
            continue
        dmasks = [torch.from_numpy(a).to(DEV) for a in masks]
        for kind in kinds:
            if kind not in grids:
                continue
            ind = grids[kind]
            where = (lc.case_id(K, L, B, h, w), kind, (c, m))
            comp = codec.compress(torch.from_numpy(ind).to(DEV), dmasks, mode)
            host = comp.to_host()
            for b in lc.checked_images(B):
                want = orc.compress_image(ind[b], masks[0][b, 0], masks[1][b, 0], masks[2][b, 0], mode, htab)
                assert host[b] == want, where + (b, {n: (len(host[b].get(n, b"")), len(want[n])) for n in want})
            exp = lc.merged_grid(ind, masks[0][:, 0], masks[1][:, 0], masks[2][:, 0])
            exp_dev = torch.from_numpy(exp).to(DEV)
            zq_want = cbk_dev[exp_dev].permute(0, 3, 1, 2)
            b0 = lc.checked_images(B)[-1]
            assert np.array_equal(orc.decompress_image(host[b0], mode, h, w, htab)[0], exp[b0]), where
            for decoder in (None, "latency", "throughput"):
                dind, dmask, zq, status = codec.decompress(comp, decoder=decoder)
                assert int(status.abs().max()) == 0, where + (decoder, status.tolist()[:8])
                bad = (dind != exp_dev).nonzero()
                assert bad.numel() == 0, where + (decoder, int(bad.shape[0]), bad[:4].tolist())
                assert all(torch.equal(a, b_) for a, b_ in zip(dmask, dmasks)), where + (decoder,)
                assert torch.equal(zq, zq_want), where + (decoder,)
            ran += 1
    return ran


def _ids(rows):
    return [lc.case_id(*r[:5]) for r in rows]


_K1024 = [r for r in lc.CODEC_CASES if r[0] == 1024 and r[1] <= 64]
_OTHER = [r for r in lc.CODEC_CASES if r not in _K1024]


@gpu
@pytest.mark.parametrize("K,L,B,h,w,paths", _K1024, ids=_ids(_K1024))
def test_batched_codec_1024_symbols(K, L, B, h, w, paths):
    """14 to 64 bits: LUT misses walk the trie (1023 nodes: staged in LDS); from 33 bits on the encoder fetches two words per code"""
    assert K - 1 <= _constant("cgic_coder_dev.h", "kLdsTrieNodes") and L <= _constant("cgic_decode_plan.h", "kSplitMaxLen")
    # a 4x4 grid holds 16 symbols: the ramp of the named lengths; every other grid holds every class
    assert _run_case(K, L, B, h, w) == len(lc.RATIOS) * len(lc.CONTENT)


@gpu
@pytest.mark.parametrize("K,L,B,h,w,paths", _OTHER, ids=_ids(_OTHER))
def test_batched_codec_other_tables(K, L, B, h, w, paths):
    """65 bits: three words per code, the serial decoder whatever the decoder argument.  2560 symbols at 64 bits: the encoder's table
    is not in LDS (beyond kLdsTable symbols, and two words), and the decode trie has a node per inner node of the code tree,
    K - 1 = 2559 > kLdsTrieNodes: it is walked in global memory.  96 symbols at 33 bits: a small table with two-word codes"""
    trie_nodes, lds_nodes = K - 1, _constant("cgic_coder_dev.h", "kLdsTrieNodes")
    assert (trie_nodes > lds_nodes) == (K == 2560) and (K > _constant("cgic_coder.hip", "kLdsTable")) == (K == 2560)
    assert (L > _constant("cgic_decode_plan.h", "kSplitMaxLen")) == (paths[0] == "serial")
    assert _run_case(K, L, B, h, w) == len(lc.RATIOS) * len(lc.CONTENT)


@gpu
@pytest.mark.parametrize("form,B,h,w,paths", lc.FORM_CASES, ids=[f"{r[0]}-{r[1]}x{r[2]}x{r[3]}" for r in lc.FORM_CASES])
def test_encoder_forms_with_the_64_bit_table(form, B, h, w, paths):
    """one case per form of the encoder that cgic_coder_plan.h distinguishes, at the smallest grid (and batch) that reaches it; the
    thresholds are the plan header's, the plan of each shape a row of tests/test_coder_plan_host.py"""
    pos_small, pos_lds, part_pos = (_constant("cgic_coder_plan.h", n) for n in ("kLdsPosSmall", "kLdsPos", "kEncPartPos"))
    max_parts, stage_max = _constant("cgic_coder_plan.h", "kEncMaxParts"), _constant("cgic_coder_plan.h", "kEncStageMax")
    one_request = _constant("cgic_decode_plan.h", "kTicketRequestMax")
    npos = h * w
    parts = min(-(-npos // part_pos), max_parts)
    want = ("lds-small" if npos <= pos_small else "lds" if npos <= pos_lds
            else ("staged" if 2 * npos <= stage_max else "global") if 6 * B > one_request
            else "parts" if 2 * ((-(-npos // parts) + 3) // 4 * 4) <= stage_max else "global")
    assert want == form
    # the long batch once, at the ratio pair with all three index streams; the others at every ratio pair
    ratios = ((0.1, 0.8),) if B > 100 else None
    assert _run_case(1024, 64, B, h, w, kinds=("uniform", "deep_short"), ratios=ratios) == 2 * (1 if ratios else len(lc.RATIOS))


def test_no_content_class_is_vacuous():
    """CPU: the cumulative code lengths of the streams the GPU cases encode.  For every table: a code of lut_bits + 1 bits, of 32, of
    33 and of the longest length, each as far as the table has it, occurs in some stream of EVERY grid that can hold them (in the
    ramp); for the 64-bit table some codeword starts at bit 0 and some at bit 63 of a 64-bit chunk of the payload, in one grid at
    least, and deep_short enters successive chunks at every offset 0 .. 63"""
    from oracle import cgic_oracle as orc
    orc.build()
    seen_63 = set()
    for K, L, B, h, w, _ in lc.CODEC_CASES:
        _, htab = _table(K, L)
        lens = htab.len.astype(np.int64)
        named = lc.named_lengths(lens)
        assert L in named and (lc.LUT_BITS + 1 in named or L >= 32) and ((32 in named and 33 in named) if L == 33 else True)
        grids = lc.grid_contents(lens, B, h, w)
        assert set(grids) == set(lc.CONTENT), "every grid of the table holds every class"
        occur, starts = set(), {k: set() for k in grids}
        for (c, m), mode, masks in _routes(B, h, w):
            for kind, ind in grids.items():
                for b in lc.checked_images(B)[:1]:
                    for sym in _streams_of(ind[b], masks, b):
                        occur |= set(lens[sym].tolist())
                        starts[kind] |= set((lc.start_bits(lens, sym) % 64).tolist())
        assert set(named) <= occur, (lc.case_id(K, L, B, h, w), named, sorted(occur))
        assert set(lens[grids["deepest"].ravel()].tolist()) == {L}
        if L == 64 and h * w >= 64 * 64:
            assert starts["deep_short"] == set(range(64)), lc.case_id(K, L, B, h, w)
            assert starts["deepest"] == {0}                       # one boundary per chunk, for ever at offset 0
            assert {0, 63} <= starts["uniform"] | starts["ramp"] | starts["deep_short"]
            seen_63.add((K, B, h, w))
    assert len(seen_63) >= 5


# ---------------------------------------------------------------------------- single-stream entry points
@gpu
@pytest.mark.parametrize("L", [33, 64, 65])
def test_single_stream_entry_points(L):
    """HuffmanCoding.encode_to_bytes / decode_bytes against the oracle's encode / decode: streams of 1 symbol up to 36 864 (beyond
    kLdsPos positions: the workspace path), around the 64 symbols of one scan step"""
    from oracle import cgic_oracle as orc
    (codec, _), (_, htab) = _codec(1024, L), _table(1024, L)
    huff = codec.huffman
    assert 36864 > _constant("cgic_coder_plan.h", "kLdsPos")
    for kind in ("uniform", "deep_short"):
        for n in (1, 2, 63, 64, 65, 4096, 36864):
            sym = lc.content_grid(kind, htab.len, (n,))
            data = huff.encode_to_bytes(torch.from_numpy(sym).to(DEV))
            want = orc.encode(htab, sym)
            assert data == want, (L, kind, n, len(data), len(want))
            assert np.array_equal(orc.decode(htab, want), sym)
            assert huff.decode_bytes(want) == sym.tolist(), (L, kind, n)


# ---------------------------------------------------------------------------- rate kernels
@gpu
@pytest.mark.parametrize("L", [33, 64, 65])
def test_rate_kernels_sum_long_code_lengths(L):
    """cgic_rate_table and cgic_rate_curve sum code lengths: the bytes they predict == the sizes of the streams compress writes at
    the same ratios == the sizes of the oracle's streams, at code lengths up to 65 bits (B = 2, a 32x48 latent)"""
    import control_gic_amd as cg
    from oracle import cgic_oracle as orc
    (codec, _), (_, htab) = _codec(1024, L), _table(1024, L)
    B, h, w = 2, 32, 48
    n16 = (h // 4) * (w // 4)
    e16n, e8n = lc.entropy_maps(B, h, w, seed=L)
    e16, e8 = torch.from_numpy(e16n).to(DEV), torch.from_numpy(e8n).to(DEV)
    up = lambda a, k: np.repeat(np.repeat(a, k, -2), k, -1)
    for kind in ("uniform", "deep_short"):
        heads = [lc.content_grid(kind, htab.len, (B, h >> s, w >> s), rng=np.random.default_rng(L + s)) for s in (2, 1, 0)]
        inds = [torch.from_numpy(a).to(DEV) for a in heads]

        def sizes(c, m):
            """[B, 5] of compress at this ratio pair, held to the oracle's streams of the oracle's masks"""
            masks, _, _, mode = cg.TripleGrainFixedEntropyRouter(c, m, per_image=True)(e16, e8, want_gate=False)
            comp = codec.compress(cg.gather_grain_indices(*inds, masks), masks, mode)
            got = comp.nbytes.clamp(min=0).cpu().numpy()
            omc, omm, omf, _, omode = orc.router(e16n, e8n, c, m, per_image=True, want_gate=False)
            assert omode == mode
            for b in range(B):
                mc, mm, mf = omc[b, 0], omm[b, 0], omf[b, 0]
                ind = np.where(mf == 1, heads[2][b], np.where(up(mm, 2) == 1, up(heads[1][b], 2), up(heads[0][b], 4)))
                st = orc.compress_image(ind, mc, mm, mf, mode, htab)
                assert got[b].tolist() == [len(st[n]) if n in st else 0 for n in orc.STREAM_NAMES], (L, kind, c, m, b)
            return got

        tab = cg.rate_table(codec, *inds, e16, e8, list(lc.RATIOS), per_image=True)
        assert tab.modes == [0, 6, 3]
        for ci, (c, m) in enumerate(lc.RATIOS):
            assert np.array_equal(tab.nbytes[ci].cpu().numpy(), sizes(c, m)), (L, kind, c, m)
        for coarse in (0.1, 0.0, 0.5):
            curve = cg.rate_curve(codec, *inds, e16, e8, coarse)
            nb = curve.nbytes.cpu().numpy()
            picks = sorted({curve.ranks[i] for i in np.linspace(0, len(curve.ranks) - 1, 6).round().astype(int)}
                           | ({cg.router_ranks(0.1, 0.8, n16)[1]} if coarse == 0.1 else set()))
            assert len(picks) >= 6
            for K in picks:
                c, m = curve.ratio(K)
                assert np.array_equal(nb[:, K], sizes(c, m)), (L, kind, coarse, K)
