"""CPU: host-side logic of the product package and the shape of the C ABI (no device compute)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import _lib
from conftest import ROOT


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "cgic_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cgic_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 25
    l = ctypes.CDLL(cg.LIB_PATH)
    for name in declared:
        assert hasattr(l, name), f"{name} declared in cgic_hip.h but not exported"
    assert declared == set(_lib.PROTOTYPES), "ctypes prototype table out of sync with the header"
    import __graft_entry__ as entry
    assert _lib.lib().cgic_abi_version() == entry.header_abi_version()


def test_graft_entry_build_passes():
    """the driver's build check: make (a no-op when the tree is built) + the ABI of the loaded library against the header"""
    import __graft_entry__ as entry
    assert entry.build() == cg.LIB_PATH


def test_device_count_does_not_abort_without_gpu():
    n = _lib.lib().cgic_device_count()
    assert n == _lib.ERR_HIP or n >= 0


class _V:
    def __init__(self, v): self.v = v
    def item(self): return self.v


@pytest.mark.parametrize("name", ["zeros", "zipf", "big", "ties"])
def test_native_table_builder_matches_reference_codes(golden, name):
    """csrc/cgic_table.hip (CPython-heapq restatement) vs the codes the reference built"""
    g = golden("coders")
    freq = g[name + "_freq"]
    order = [str(i) for i in g[name + "_order"]]
    h = cg.HuffmanCoding({k: _V(float(freq[int(k)])) for k in order})       # mapping iterated in ParameterDict order
    ln, cd = h.table.arrays()
    assert np.array_equal(np.array(ln, np.int32), g[name + "_len"])
    assert np.array_equal(np.array(cd, np.uint32), g[name + "_code"])
    hn = cg.HuffmanCoding({str(i): _V(float(v)) for i, v in enumerate(freq)})  # plain-dict order
    assert np.array_equal(np.array(hn.table.arrays()[0], np.int32), g[name + "_natural_len"])
    codes = h.codes
    assert len(codes) == 1024 and len(set(codes.values())) == 1024
    assert h.reverse_mapping[codes[17]] == 17
    # prefix-free
    srt = sorted(codes.values())
    assert all(not b.startswith(a) for a, b in zip(srt, srt[1:]))


def test_counter_view_iterates_like_parameter_dict():
    vq = cg.VectorQuantizer(1024, 4, beta=0.25)
    ref = torch.nn.ParameterDict({str(i): torch.nn.Parameter(torch.zeros(1)) for i in range(1024)})
    assert list(vq.embedding_counter.keys()) == list(ref.keys())
    vq.embedding_counter["7"] += 3
    vq.embedding_counter["12"].data.fill_(5.0)
    assert vq.embedding_counter["7"].item() == 3.0 and vq.usage_counter[12].item() == 5.0
    h = cg.HuffmanCoding(vq.embedding_counter)
    assert h.table.n == 1024


def test_vq_state_dict_keys_match_reference():
    vq = cg.VectorQuantizer(1024, 4, beta=0.25)
    vq.usage_counter[5] = 9.0
    sd = vq.state_dict()
    assert set(sd) == {"embedding.weight"} | {f"embedding_counter.{i}" for i in range(1024)}
    assert tuple(sd["embedding_counter.5"].shape) == (1,) and sd["embedding_counter.5"].item() == 9.0
    vq2 = cg.VectorQuantizer(1024, 4, beta=0.25)
    missing, unexpected = vq2.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert torch.equal(vq2.embedding.weight, vq.embedding.weight) and vq2.usage_counter[5].item() == 9.0
    # nested prefix, like model.quantize.*
    wrap = torch.nn.Module()
    wrap.quantize = cg.VectorQuantizer(1024, 4, beta=0.25)
    wrap.load_state_dict({"quantize." + k: v for k, v in sd.items()}, strict=True)
    assert wrap.quantize.usage_counter[5].item() == 9.0


def test_router_modes_and_streams():
    R = cg.TripleGrainFixedEntropyRouter
    assert R(0.7, 0.3).mode == 0 and R(0.3, 0.7).mode == 3        # float64 quirk, RouterTriple.py:13
    assert [R(c, m).mode for c, m in ((.1, .8), (0, .4), (.4, 0), (1, 0), (0, 1), (0, 0))] == [0, 1, 2, 4, 5, 6]
    assert R(0.1, 0.8).fine_grain_ratio == 1 - 0.1 - 0.8
    want = {0: "11111", 1: "01101", 2: "10110", 3: "11010", 4: "10000", 5: "01000", 6: "00100"}
    for mode, bits in want.items():
        assert "".join("1" if b else "0" for b in cg.mode_streams(mode)) == bits
    with pytest.raises(cg.CgicError):
        cg.mode_streams(7)


def test_product_path_refuses_cpu_tensors():
    """no CPU fallback: every op raises on CPU tensors instead of computing something else"""
    vq = cg.VectorQuantizer(1024, 4, beta=0.25)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vq(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cg.TripleGrainFixedEntropyRouter(0.1, 0.8)(torch.zeros(1, 4, 4), torch.zeros(1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cg.Entropy(8)(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cg.BinaryCoding().compress(torch.zeros(8, dtype=torch.int32), "/tmp/_never_written.bin")
    with pytest.raises(NotImplementedError):
        cg.Entropy(4)


def test_argument_validation_happens_before_any_launch():
    l = _lib.lib()
    assert l.cgic_vq_forward_f32(None, 1, 16, None, 1024, 4, 0.25, 1, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID
    one = ctypes.c_void_p(16)
    assert l.cgic_vq_forward_f32(one, 1, 16, one, 1024, 3, 0.25, 1, None, None, None, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
    assert b"embed_dim == 4" in l.cgic_last_error()
    assert l.cgic_vq_forward_f32(one, 1, 16, one, 1000, 4, 0.25, 1, None, None, None, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
    conv = _lib.Conv1x1(None, None, 0)
    assert l.cgic_vq_forward_f32(one, 1, 16, one, 1024, 4, 0.25, 1, None, None, None, None, None, ctypes.byref(conv), None, None) == _lib.ERR_INVALID      # quant_conv without a weight
    assert l.cgic_vq_backward_f32(one, 1, 16, one, 1024, 4, None, None, None, 0.25, 1, None, None, None, None) == _lib.ERR_INVALID
    assert l.cgic_vq_backward_f32(one, 1, 16, one, 1024, 4, one, None, None, 0.25, 1, None, one, None, None) == _lib.ERR_INVALID          # codebook gradient without workspace
    # router: k > n is an IndexError in the reference
    assert l.cgic_router_f32(one, one, 1, 4, 4, 1.5, 0.0, 0, one, one, one, None, None, None, None) == _lib.ERR_INVALID
    assert b"IndexError" in l.cgic_last_error()
    bins = (ctypes.c_float * 32)(*np.linspace(-1, 1, 32, dtype=np.float32))
    # router refinement (round 4): the kernel recomputes torch.linspace(-1, 1, 32) itself, so the caller's bins must be THE
    # linspace to the bit (numpy's differs from torch's in the second half); segments that do not fit the LDS are refused
    tb = _lib.linspace_bins()
    # the two calls that pass validation go on to launch: where a device exists they get real buffers (maps, masks, pixels of
    # one 64x64 image) -- a launch on made-up addresses would read and write them on the GPU; without one the launch fails
    if torch.cuda.is_available():
        dev = torch.device("cuda", 0)
        bufs = [torch.rand(1, 4, 4, device=dev), torch.rand(1, 8, 8, device=dev)] + \
               [torch.zeros(1, n, n, dtype=torch.int32, device=dev) for n in (4, 8, 16)] + [torch.rand(1, 3, 64, 64, device=dev)]
        e16, e8, mc, mm, mf = (ctypes.c_void_p(b.data_ptr()) for b in bufs[:5])
        x, launched = bufs[5].data_ptr(), (_lib.OK,)
    else:
        e16 = e8 = mc = mm = mf = one
        x, launched = 16, (_lib.ERR_HIP, _lib.OK)
    px = _lib.Pixels(x, 0, tb, 32, 0.01, None)
    assert l.cgic_router_f32(e16, e8, 1, 4, 4, 0.1, 0.8, 1, mc, mm, mf, None, None, ctypes.byref(px), None) in launched  # passes validation
    bad = (ctypes.c_float * 32)(*[v + (1e-7 if i == 20 else 0.0) for i, v in enumerate(tb)])
    assert l.cgic_router_f32(one, one, 1, 4, 4, 0.1, 0.8, 1, one, one, one, None, None, ctypes.byref(_lib.Pixels(16, 0, bad, 32, 0.01, None)), None) == _lib.ERR_UNSUPPORTED
    assert b"linspace" in l.cgic_last_error()
    # a segment beyond the LDS (the flattened batch of 64: the reference's encode() semantics) is refined through patched copies of
    # the maps (ABI 8) and REQUIRES the scratch: without it the call is refused, never routed from unrefined maps
    assert l.cgic_router_f32(one, one, 64, 16, 16, 0.1, 0.8, 0, one, one, one, None, None, ctypes.byref(px), None) == _lib.ERR_INVALID
    assert b"cgic_router_refine_scratch_bytes" in l.cgic_last_error()
    assert l.cgic_router_refine_supported(64, 16, 16, 1) == 1 and l.cgic_router_refine_supported(8, 48, 48, 1) == 1
    assert l.cgic_router_refine_supported(64, 16, 16, 0) == 1 and l.cgic_router_refine_supported(1, 128, 85, 1) == 1
    assert l.cgic_router_refine_in_lds(64, 16, 16, 1) == 1 and l.cgic_router_refine_in_lds(8, 48, 48, 1) == 1 and l.cgic_router_refine_in_lds(8, 16, 16, 0) == 1
    assert l.cgic_router_refine_in_lds(64, 16, 16, 0) == 0 and l.cgic_router_refine_in_lds(1, 128, 85, 1) == 0
    assert l.cgic_router_refine_scratch_bytes(64, 16, 16, 0) == 20 * 64 * 256 + 16 + 64
    assert l.cgic_router_f32(e16, e8, 1, 4, 4, 1.0, 0.0, 1, mc, mm, mf, None, None, ctypes.byref(_lib.Pixels(x, 0, bad, 32, 0.01, None)), None) in launched  # mode 4 compares nothing: pixels ignored
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    assert l.cgic_entropy_maps_f32(one, 1, 24, 32, bins, 32, 0.01, one, one, None, None) == _lib.ERR_INVALID
    assert l.cgic_entropy_maps_f32(one, 1, 32, 32, bins, 32, 0.05, one, one, None, None) == _lib.ERR_UNSUPPORTED


def test_slot_and_workspace_sizes():
    h = cg.HuffmanCoding({str(i): _V(float(1024 - i)) for i in range(1024)})
    l = _lib.lib()
    slot = l.cgic_compress_slot_bytes(h.table.handle, 64, 64)
    assert slot % 16 == 0 and slot >= 4096 * h.table.max_len // 8 + 2
    assert l.cgic_compress_workspace_bytes(64, 64, 64) == 0                 # 4096 positions fit LDS
    assert l.cgic_compress_workspace_bytes(1, 192, 192) >= 3 * 36864 * 6    # 768^2 tile: global scratch
    assert l.cgic_decompress_workspace_bytes(2, 64, 64) >= 2 * (256 + 1024 + 4096) * 2 + 24   # u16 symbols + counts


def test_custom_ops_schema_and_fake_tensor_shapes():
    """torch.ops.cgic.*: registered with a schema and shape inference (what torch.compile / FakeTensor need); no kernel runs.
    A CPU tensor has no implementation -- there is no CPU fallback."""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "Tensor z, Tensor codebook, float beta, bool legacy" in str(torch.ops.cgic.vq_forward.default._schema)
    with FakeTensorMode():
        z, cb = torch.empty(2, 4, 16, 24, device="cuda"), torch.empty(1024, 4, device="cuda")
        zq, loss, idx = torch.ops.cgic.vq_forward(z, cb, 0.25, True)
        assert tuple(zq.shape) == (2, 4, 16, 24) and loss.shape == () and tuple(idx.shape) == (768,) and idx.dtype == torch.int64
        e8, e16 = torch.ops.cgic.entropy_maps(torch.empty(2, 3, 64, 96, device="cuda"))
        assert tuple(e8.shape) == (2, 8, 12) and tuple(e16.shape) == (2, 4, 6)
        masks = torch.ops.cgic.router(e16, e8, 0.1, 0.8, True)
        assert [tuple(m.shape) for m in masks] == [(2, 1, 4, 6), (2, 1, 8, 12), (2, 1, 16, 24)] and masks[0].dtype == torch.int32
        xf, f8, f16 = torch.ops.cgic.entropy_maps_u8(torch.empty(2, 64, 96, 3, device="cuda", dtype=torch.uint8))
        assert tuple(xf.shape) == (2, 3, 64, 96) and xf.dtype == torch.float32 and tuple(f8.shape) == (2, 8, 12) and tuple(f16.shape) == (2, 4, 6)
        out = torch.ops.cgic.vq_forward_route(z, cb, 0.25, True, torch.empty(2, 4, 6, device="cuda"), torch.empty(2, 8, 12, device="cuda"), 0.1, 0.8, True)
        assert len(out) == 6 and tuple(out[5].shape) == (2, 1, 16, 24)
        gz, gw = torch.ops.cgic.vq_backward(z, cb, idx, zq, loss, 0.25, True)
        assert gz.shape == z.shape and gw.shape == cb.shape
    with pytest.raises(NotImplementedError):
        torch.ops.cgic.vq_forward(torch.zeros(1, 4, 4, 4), torch.zeros(1024, 4), 0.25, True)


def test_codec_and_merge_custom_ops_schema_and_fake_tensor_shapes():
    """(round-2 verdict item 5) the codec, the single-stream coders, the histogram and the mask-merge kernels are PyTorch custom
    ops too: schema + FakeTensor shapes (stream slots sized by cgic_compress_slot_bytes), no kernel runs here"""
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import control_gic_amd as cg
    freq = {str(i): float(1024 - i) for i in range(1024)}
    huff = cg.HuffmanCoding(freq)
    table = huff.table.handle.value
    slot = cg._lib.lib().cgic_compress_slot_bytes(huff.table.handle, 16, 24)
    for name in ("compress_streams", "decompress_streams", "encode_stream", "decode_stream", "index_histogram", "grain_merge", "avg_pool",
                 "decoder_blend_medium", "decoder_blend_fine"):
        assert hasattr(torch.ops.cgic, name), name
    assert "Tensor(a6!)? hist" in str(torch.ops.cgic.compress_streams.default._schema)          # the histogram is mutated in place
    assert "str decoder" in str(torch.ops.cgic.decompress_streams.default._schema)              # the decoder is a per-call argument
    with FakeTensorMode():
        dev = "cuda"
        ind = torch.empty(2 * 16 * 24, dtype=torch.int64, device=dev)
        mk = lambda s: torch.empty(2, 1, 16 // s, 24 // s, dtype=torch.int32, device=dev)
        data, nbytes = torch.ops.cgic.compress_streams(ind, mk(4), mk(2), mk(1), 0, table, None)
        assert tuple(data.shape) == (2, 5, slot) and data.dtype == torch.uint8 and tuple(nbytes.shape) == (2, 5) and nbytes.dtype == torch.int32
        cb = torch.empty(1024, 4, device=dev)
        out = torch.ops.cgic.decompress_streams(data, nbytes, 16, 24, 0, table, cb, "throughput")
        assert [tuple(t.shape) for t in out] == [(2, 16, 24), (2, 1, 4, 6), (2, 1, 8, 12), (2, 1, 16, 24), (2, 4, 16, 24), (2,)]
        assert out[0].dtype == torch.int64 and out[4].dtype == torch.float32 and out[5].dtype == torch.int32
        b, n = torch.ops.cgic.encode_stream(torch.empty(100, dtype=torch.int64, device=dev), table)
        assert b.dtype == torch.uint8 and b.numel() == cg._lib.lib().cgic_stream_capacity(huff.table.handle, 100) and tuple(n.shape) == (1,)
        syms, cnt = torch.ops.cgic.decode_stream(torch.empty(64, dtype=torch.uint8, device=dev), 40, table)
        assert tuple(syms.shape) == (39 * 8,) and syms.dtype == torch.int64 and tuple(cnt.shape) == (1,)
        hf = torch.empty(2, 8, 16, 24, device=dev)
        hm, hc = torch.empty(2, 8, 8, 12, device=dev), torch.empty(2, 8, 4, 6, device=dev)
        assert tuple(torch.ops.cgic.grain_merge(hc, hm, hf, mk(4), mk(2), mk(1)).shape) == (2, 8, 16, 24)
        assert tuple(torch.ops.cgic.avg_pool(hf, 4).shape) == (2, 8, 4, 6) and tuple(torch.ops.cgic.avg_pool(hf, 2).shape) == (2, 8, 8, 12)
        assert tuple(torch.ops.cgic.decoder_blend_medium(hm, hm, mk(4), mk(2)).shape) == (2, 8, 8, 12)
        assert tuple(torch.ops.cgic.decoder_blend_fine(hf, hf, mk(4), mk(2), mk(1)).shape) == (2, 8, 16, 24)
    with pytest.raises(NotImplementedError):
        torch.ops.cgic.avg_pool(torch.zeros(1, 1, 4, 4), 2)


def test_byte_over_255_formula_of_the_uint8_entropy_kernel_is_torchs_division():
    """cgic_entropy_maps_u8 converts a byte with q = b * fl(1/255); q = fma(fma(-q, 255, b), fl(1/255), q) (unit_of_byte,
    cgic_entropy.hip): for every byte that is the fp32 quotient torch's `.div(255)` (T.ToTensor(), inference.py:50-53) produces.
    The fmas are emulated in float64 (products of fp32 values and these sums are exact there)."""
    import torch
    b = np.arange(256, dtype=np.float32)
    ref = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).numpy()
    r = np.float32(0.00392156886)
    assert r == np.float32(1) / np.float32(255)
    q = (b * r).astype(np.float32)
    e = (b.astype(np.float64) - q.astype(np.float64) * 255.0)
    assert np.array_equal(e, e.astype(np.float32).astype(np.float64))               # the remainder is an fp32 number: the fma is exact
    q2 = (e * np.float64(r) + q.astype(np.float64)).astype(np.float32)
    assert np.array_equal(q2, ref)
    assert int((q != ref).sum()) > 100                                              # the plain product is NOT the quotient


def test_codec_follows_the_counters_and_refuses_a_foreign_table():
    """model._codec_for (behind compress / compress_batch): the Huffman table is rebuilt when embedding_counter changed (a
    training step between two compress() calls; round 3 kept the stale table), and a coder handed in as h_indices must carry
    the code of these counters -- a foreign coder with another table raises instead of being silently ignored"""
    import types
    from control_gic_amd import model as cm
    vq = cg.VectorQuantizer(1024, 4, beta=0.25)
    vq.usage_counter.copy_(torch.arange(1024, 0, -1, dtype=torch.float32))
    m = types.SimpleNamespace(quantize=vq)
    c1 = cm._codec_for(m)
    assert cm._codec_for(m) is c1                                   # unchanged counters: cached
    codes1 = dict(c1.huffman.codes)
    with torch.no_grad():
        vq.usage_counter[5] += 4000.0                              # (what fold_usage_hist does in training)
    c2 = cm._codec_for(m)
    assert c2 is not c1 and c2.huffman.codes != codes1
    assert c2.huffman.codes == cg.HuffmanCoding(vq.embedding_counter).codes
    own = cg.HuffmanCoding(vq.embedding_counter)
    assert cm._codec_for(m, own).huffman is own                     # a control_gic_amd coder is used as it is
    same = types.SimpleNamespace(codes={k: v for k, v in c2.huffman.codes.items()})     # the reference's class: .codes {symbol: bits}
    cm._codec_for(m, same)
    other = types.SimpleNamespace(codes=codes1)
    with pytest.raises(ValueError, match="code table"):
        cm._codec_for(m, other)
    with pytest.raises(ValueError, match="code table"):
        cm._codec_for(m, object())


def test_cluster_packing_fills_tiles_exactly_where_the_sizes_allow():
    """round 6: cgic_vq_prepare_f32 packs near-duplicate rows (a trained codebook's clusters, quantize.py:22-26) into 32-code tiles;
    the packing itself is host code (cgic_vq_cluster_permutation_host).  On the bench's clustered codebook (64 centres, cluster
    sizes 9..25) every tile is filled to exactly 32 rows and at most 2 clusters are cut (first fit, largest first, cut 7); a
    codebook without near-duplicates has nothing to pack; K=1024 singles + a few pairs stay whole."""
    import ctypes
    from control_gic_amd import _lib
    l = _lib.lib()
    rng = np.random.default_rng(77)
    centres = rng.standard_normal((64, 4), dtype=np.float32)
    assign = rng.integers(0, 64, 1024)
    cb = (centres[assign] + np.float32(1e-4) * rng.standard_normal((1024, 4), dtype=np.float32)).astype(np.float32)
    perm = np.zeros(1024, np.uint16)
    rc = l.cgic_vq_cluster_permutation_host(cb.ctypes.data_as(ctypes.c_void_p), 1024, perm.ctypes.data_as(ctypes.c_void_p))
    assert rc == 1 and sorted(perm.tolist()) == list(range(1024))
    tile_of = np.empty(1024, np.int64)
    tile_of[perm] = np.arange(1024) // 32
    cut = [c for c in range(64) if len(set(tile_of[assign == c].tolist())) > 1]
    assert len(cut) <= 2, cut
    # nothing to pack
    plain = np.random.default_rng(1).standard_normal((1024, 4)).astype(np.float32)
    assert l.cgic_vq_cluster_permutation_host(plain.ctypes.data_as(ctypes.c_void_p), 1024, perm.ctypes.data_as(ctypes.c_void_p)) == 0
    # a few duplicated rows among singles: every pair / triple ends up inside one tile
    dup = plain.copy()
    dup[100] = dup[7]; dup[900] = dup[7]; dup[512] = dup[33]
    assert l.cgic_vq_cluster_permutation_host(dup.ctypes.data_as(ctypes.c_void_p), 1024, perm.ctypes.data_as(ctypes.c_void_p)) == 1
    tile_of[perm] = np.arange(1024) // 32
    assert tile_of[100] == tile_of[7] == tile_of[900] and tile_of[512] == tile_of[33] and sorted(perm.tolist()) == list(range(1024))
    assert l.cgic_vq_cluster_permutation_host(None, 1024, perm.ctypes.data_as(ctypes.c_void_p)) == _lib.ERR_INVALID
