"""GPU: the self-synchronising decoder's wave-local fix point, its one-barrier scan and the one-band merge, at their edges.

With at most one 64-bit chunk per lane (every case here: the chunk count is asserted on the CPU) each wave of decode_image_kernel
iterates on its own chunks and meets the others only when it is locally stable; the cases put chunk counts, stream starts, payload
ends and sweep counts where that loop, the prefix of the counts and the merge's first-band shortcut take another path.  Every case is
a batch of 3 images that differ, through GrainCodec.decompress under decoder_mode("throughput"), and every comparison is equality:

  decoded indices == oracle.cgic_oracle.decompress_image of the same bytes, image by image;
  indices, masks, codebook rows and status == the latency decoder's;
  cgic_decode_stats counted one image-decoder workgroup per image (the path under test really ran)."""
import functools

import numpy as np
import pytest
import torch

import long_codes_ref as lc

DEV = "cuda"
pytestmark = pytest.mark.gpu
B = 3
MAX_SWEEPS = 32                    # kSsMaxSweeps of csrc/cgic_decode_ss.hip
LANES = 256                        # kSsThreadsSmall: the workgroup of these grids


class _V:
    def __init__(self, v): self.v = v
    def item(self): return self.v


@functools.lru_cache(maxsize=None)
def _coder(name):
    """(codec, oracle table, code lengths) of the trained model's Zipf-like table (longest code 13 bits), of the table of equal
    counts (every code 10 bits) or of the ladder with a longest code of 14 bits (LUT misses continue in the trie)"""
    import control_gic_amd as cg
    from conftest import load_golden
    from oracle import cgic_oracle as orc
    orc.build()
    if name == "zipf":
        freq = load_golden("coders")["zipf_freq"]
    elif name == "equal":
        freq = np.full(1024, 7.0)
    else:
        freq = lc.ladder_table(1024, 14)
    htab = orc.HuffmanTable(freq)
    cbk = np.random.default_rng(len(name)).standard_normal((1024, 4)).astype(np.float32)
    codec = cg.GrainCodec({str(int(s)): _V(float(freq[int(s)])) for s in orc.param_dict_order(1024)}, torch.from_numpy(cbk).to(DEV))
    lens = np.asarray(htab.len, np.int64)
    assert codec.huffman.table.max_len == int(lens.max())
    return codec, htab, lens


def _route(h, w, c, m, seed):
    from oracle import cgic_oracle as orc
    e16, e8 = lc.entropy_maps(B, h, w, seed)
    mc, mm, mf, _, mode = orc.router(e16, e8, c, m, per_image=True, want_gate=False)
    return (mc, mm, mf), mode


def _stream_bits(lens, ind, masks, b):
    """payload bits of image b's coarse, medium and fine index streams"""
    from oracle import cgic_oracle as orc
    return [int(lens[s].sum()) for s in orc.select(ind[b], masks[0][b, 0], masks[1][b, 0], masks[2][b, 0])]


def _chunks(bits):
    return [(v + 63) // 64 for v in bits]


def _decode_and_compare(name, ind, masks, mode):
    """-> (sum, images, max) of the decoder's sweep counters"""
    import control_gic_amd as cg
    from oracle import cgic_oracle as orc
    codec, htab, lens = _coder(name)
    h, w = ind.shape[1:]
    for b in range(B):
        assert 1 <= sum(_chunks(_stream_bits(lens, ind, masks, b))) <= LANES, "one chunk per lane at the most"
    dmasks = [torch.from_numpy(a).to(DEV) for a in masks]
    comp = codec.compress(torch.from_numpy(ind).to(DEV), dmasks, mode)
    host = comp.to_host()
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    lib = cg._lib.lib()
    assert lib.cgic_decode_stats(cnt.data_ptr()) == 0
    try:
        with cg.decoder_mode("throughput"):
            dind, dmask, zq, status = codec.decompress(comp)
        torch.cuda.synchronize()
    finally:
        lib.cgic_decode_stats(None)
    cnt = cnt.tolist()
    assert cnt[1] == B, cnt
    assert int(status.abs().max()) == 0, status.tolist()
    got = dind.cpu().numpy()
    exp = lc.merged_grid(ind, masks[0][:, 0], masks[1][:, 0], masks[2][:, 0])
    for b in range(B):
        assert host[b] == orc.compress_image(ind[b], masks[0][b, 0], masks[1][b, 0], masks[2][b, 0], mode, htab), (name, mode, b)
        want = orc.decompress_image(host[b], mode, h, w, htab)[0]
        assert np.array_equal(want, exp[b]), (name, mode, b)
        bad = np.argwhere(got[b] != want)
        assert bad.size == 0, (name, mode, b, len(bad), bad[:4].tolist())
    lind, lmask, lzq, lstatus = codec.decompress(comp, decoder="latency")
    assert torch.equal(dind, lind) and torch.equal(zq, lzq) and torch.equal(status, lstatus)
    assert all(torch.equal(a, b_) for a, b_ in zip(dmask, lmask)) and all(torch.equal(a, b_) for a, b_ in zip(dmask, dmasks))
    return cnt[0], cnt[1], cnt[2]


def _with_total(lens, n, total):
    """n symbols whose code lengths add up to `total` bits"""
    avail = sorted(set(lens.tolist()))
    lo = avail[0]
    deficit = total - n * lo
    assert deficit >= 0
    out = []
    for _ in range(n):
        pick = max(v for v in avail if v - lo <= deficit)
        deficit -= pick - lo
        out.append(int(np.flatnonzero(lens == pick)[0]))
    assert deficit == 0 and int(lens[out].sum()) == total
    return np.array(out, np.int64)


def test_one_chunk_per_stream():
    """an 8x4 grid with the shortest codes: three streams of one chunk each, three lanes of one wave at work"""
    _, _, lens = _coder("zipf")
    short = np.argsort(lens, kind="stable")[:8]
    ind = short[np.random.default_rng(1).integers(0, 8, (B, 8, 4))]
    masks, mode = _route(8, 4, 0.75, 0.1, seed=84)
    assert mode == 0
    per_image = [_chunks(_stream_bits(lens, ind, masks, b)) for b in range(B)]
    assert all(c == [1, 1, 1] for c in per_image), per_image
    _decode_and_compare("zipf", ind, masks, mode)


def test_all_fine_stream_crosses_two_wave_boundaries():
    """32x32, every position fine: one stream of about 190 chunks, lanes of three waves"""
    _, _, lens = _coder("zipf")
    ind = np.random.default_rng(2).integers(0, 1024, (B, 32, 32))
    masks, mode = _route(32, 32, 0.0, 0.0, seed=3232)
    assert mode == 6
    for b in range(B):
        c = _chunks(_stream_bits(lens, ind, masks, b))
        assert c[0] == 0 and c[1] == 0 and 128 < c[2] <= 192, c
    total, _, most = _decode_and_compare("zipf", ind, masks, mode)
    assert B <= total and most <= MAX_SWEEPS, (total, most)


def test_stream_that_never_resynchronises_reaches_the_all_entries_pass():
    """one 13-bit codeword repeated (13 and 64 are coprime: a wrong entry offset stays wrong): the sweeps run out in every wave and
    the all-entries pass finishes; the other two images are a second such stream and an ordinary one"""
    _, _, lens = _coder("zipf")
    deep = np.flatnonzero(lens == 13)
    assert lens.max() == 13 and len(deep) >= 2
    ind = np.random.default_rng(3).integers(0, 1024, (B, 32, 32))
    ind[0] = deep[0]
    ind[1] = deep[-1]
    masks, mode = _route(32, 32, 0.0, 0.0, seed=13)
    assert mode == 6 and _chunks(_stream_bits(lens, ind, masks, 0))[2] == 208
    _, _, most = _decode_and_compare("zipf", ind, masks, mode)
    assert most > MAX_SWEEPS, most


def test_equal_code_lengths():
    """every code 10 bits: the guess has to lie in the residue class of the lengths' gcd, and is then right at once"""
    _, _, lens = _coder("equal")
    assert set(lens.tolist()) == {10}
    ind = np.random.default_rng(4).integers(0, 1024, (B, 32, 32))
    for (c, m), want_mode in (((0.0, 0.0), 6), ((0.1, 0.8), 0)):
        masks, mode = _route(32, 32, c, m, seed=10)
        assert mode == want_mode
        _decode_and_compare("equal", ind, masks, mode)


def test_payload_ends_on_and_just_behind_a_chunk_boundary():
    """16x8 all fine: 128 codewords of 1280 bits (20 chunks, the last one full), of 1281 bits (one bit in chunk 21) and of 1279"""
    _, _, lens = _coder("zipf")
    ind = np.stack([_with_total(lens, 128, t)[np.random.default_rng(t).permutation(128)].reshape(16, 8) for t in (1280, 1281, 1279)])
    masks, mode = _route(16, 8, 0.0, 0.0, seed=64)
    assert mode == 6
    assert [_stream_bits(lens, ind, masks, b)[2] for b in range(B)] == [1280, 1281, 1279]
    _decode_and_compare("zipf", ind, masks, mode)


def test_stream_starts_inside_a_wave():
    """32x32: medium and fine streams only (no coarse stream: stream 1 starts at chunk 0), then all three present, their first
    chunks on lanes inside a wave"""
    _, _, lens = _coder("zipf")
    ind = np.random.default_rng(5).integers(0, 1024, (B, 32, 32))
    seen = []
    for c, m in ((0.0, 0.5), (0.1, 0.8)):
        masks, mode = _route(32, 32, c, m, seed=55)
        ch = [_chunks(_stream_bits(lens, ind, masks, b)) for b in range(B)]
        seen.append((mode, ch))
        _decode_and_compare("zipf", ind, masks, mode)
    (mode_a, ch_a), (mode_b, ch_b) = seen
    assert mode_a == 1 and all(c[0] == 0 and c[1] > 0 and c[2] > 0 and c[1] % 64 for c in ch_a), seen
    assert mode_b == 0 and all(min(c) > 0 and c[0] % 64 and (c[0] + c[1]) % 64 for c in ch_b), seen


def test_trie_table_is_unchanged():
    """longest code 14 bits: beyond the LUT window, so a walk continues in the trie and no all-entries pass exists"""
    _, _, lens = _coder("ladder14")
    assert lens.max() == 14 > lc.LUT_BITS
    grids = lc.grid_contents(lens, B, 32, 32)
    for kind, (c, m) in (("uniform", (0.0, 0.0)), ("deep_short", (0.1, 0.8)), ("ramp", (0.1, 0.8))):
        masks, mode = _route(32, 32, c, m, seed=14)
        _decode_and_compare("ladder14", grids[kind], masks, mode)


@pytest.mark.parametrize("c,m,want_mode", [(0.1, 0.8, 0), (0.0, 0.5, 1), (0.5, 0.0, 2), (0.5, 0.5, 3), (1.0, 0.0, 4), (0.0, 1.0, 5), (0.0, 0.0, 6)])
def test_one_band_merge_in_every_mode(c, m, want_mode):
    """16x16 latents: one workgroup merges the whole image (its first row is row 0) in each of the seven routing modes"""
    ind = np.random.default_rng(60 + want_mode).integers(0, 1024, (B, 16, 16))
    masks, mode = _route(16, 16, c, m, seed=160 + want_mode)
    assert mode == want_mode
    _decode_and_compare("zipf", ind, masks, mode)
