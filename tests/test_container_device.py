"""The container built and loaded on the device (csrc/cgic_container.hip: container.pack_device / container.load) against the CPU
reference: container.pack / container.unpack on to_host() results, which the fixtures of the other test files pin to the reference's
bytes.  Small shapes on purpose: 64x64-pixel images (16x16 latents), an 80x112 image cut with tile=64 (four tile shapes), and one
768x768 tile for a stream far longer than one workgroup's share of the copy."""
import numpy as np
import pytest
import torch

import control_gic_amd as cg
from control_gic_amd import container, highres
from control_gic_amd.quantize import vq_forward_route

pytestmark = pytest.mark.gpu
DEV = "cuda"
RATIOS = ((0.1, 0.8), (0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0))      # test_grain_merge_bit_exact's: modes 0 .. 6
EMPTY_COARSE = (0.02, 0.9)          # mode 0 with round(16 x 0.02) = 0 coarse patches: indices_coarse is written and empty
FREQ = np.floor(1e6 / (1 + np.arange(1024)) ** 1.1).astype(np.int64)                           # Zipf-like


@pytest.fixture(scope="module")
def kit():
    vq = cg.VectorQuantizer(1024, 4, beta=0.25).to(DEV).eval()
    with torch.no_grad():
        vq.embedding.weight.copy_(torch.from_numpy(np.random.default_rng(1).standard_normal((1024, 4)).astype(np.float32)))
    vq.usage_counter.copy_(torch.from_numpy(FREQ.astype(np.float32)))
    return vq, cg.GrainCodec(vq.embedding_counter, vq.embedding.weight.detach())


def _inputs(B, H, W, seed):
    """indices drawn from the table's own distribution and two entropy maps, as host arrays"""
    rng = np.random.default_rng(seed)
    ind = rng.choice(1024, size=(B, H // 4, W // 4), p=FREQ / FREQ.sum()).astype(np.int64)
    return ind, (rng.random((B, H // 16, W // 16)) * 2.6).astype(np.float32), (rng.random((B, H // 8, W // 8)) * 2.6).astype(np.float32)


def _compress(codec, B, H, W, ratio, seed):
    ind, e16, e8 = _inputs(B, H, W, seed)
    mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(*ratio, per_image=True)(torch.from_numpy(e16).to(DEV), torch.from_numpy(e8).to(DEV))
    return codec.compress(torch.from_numpy(ind).to(DEV), mask, mode)


_cache = {}


def _batch(kit, ratio, B=3, seed=11):
    """(CompressedBatch, its reference blob) of B images of 64x64, made once per ratio and left unchanged"""
    key = (ratio, B, seed)
    if key not in _cache:
        comp = _compress(kit[1], B, 64, 64, ratio, seed)
        _cache[key] = (comp, container.pack(container.entries_from_batch(comp, 64, 64)))
    return _cache[key]


def _encode(vq):
    def encode(tiles):                      # a stand-in encoder that is a function of each tile's own pixels
        z = torch.nn.functional.avg_pool2d(tiles, 4)
        z = torch.cat([z, z[:, :1] * 2 - 1], dim=1) * 3 - 1.5
        e8, e16 = cg.entropy_maps(tiles)
        _, _, ind, mask, _, mode = vq_forward_route(z.contiguous(), vq.embedding.weight, 0.25, True, e16, e8, 0.1, 0.8, per_image=True)
        return ind, mask, mode
    return encode


def _ragged(kit):
    """two 80x112 images cut with tile=64 (tiles 64x64, 64x48, 16x64, 16x48: four shape groups, row-major order interleaves them):
    (x, one TiledImage of image 0, the list of compress_tiled_batch)"""
    if "ragged" not in _cache:
        x = torch.from_numpy((np.random.default_rng(5).integers(0, 256, (2, 3, 80, 112)) / 255.0).astype(np.float32)).to(DEV)
        one = highres.compress_tiled(x[:1], _encode(kit[0]), kit[1], tile=64)
        many = highres.compress_tiled_batch(x, _encode(kit[0]), kit[1], tile=64)
        _cache["ragged"] = (x, one, many)
    return _cache["ragged"]


def _prefilled(nbytes, guard=0):
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[:nbytes]


# ---- 1. whole images, all seven modes + an empty stream --------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", RATIOS + (EMPTY_COARSE,), ids=lambda r: f"c{r[0]}-m{r[1]}")
def test_whole_images_equal_the_cpu_container(kit, ratio):
    comp, want = _batch(kit, ratio)
    if ratio == EMPTY_COARSE:
        assert int((comp.nbytes == 0).sum()) > 0, "this case is here for its zero-length stream"
    else:
        assert comp.mode == RATIOS.index(ratio)
    _, blob = _prefilled(len(want) + 1000)
    total = torch.full((1,), -77, dtype=torch.int64, device=DEV)
    packed = container.pack_device(comp, 64, 64, blob=blob, total=total)
    assert packed.blob is blob and packed.total is total
    assert packed.nbytes() == len(want) and packed.tobytes() == want
    assert bool((blob[len(want):] == 0xA5).all()), "bytes past `total` were written"
    # the default capacity, the conveniences and other ids
    assert container.pack_device(comp, 64, 64).tobytes() == want and comp.pack(64, 64).tobytes() == want
    assert comp.pack(64, 64, first_image_id=9).tobytes() == container.pack(container.entries_from_batch(comp, 64, 64, 9))
    assert container.unpack(packed.tobytes()) == container.entries_from_batch(comp, 64, 64)


# ---- 2. alignment --------------------------------------------------------------------------------------------------------------
def test_every_payload_start_and_every_stream_residue(kit):
    comp, _ = _batch(kit, RATIOS[0])
    entries = container.entries_from_batch(comp, 64, 64)
    assert container.pack_groups([comp], []).tobytes() == container.pack([])
    # E = 0 .. 4 entries out of one batch (an image may be named twice): the payload starts at 12, 56, 100, 144, 188
    for picks in ([], [2], [0, 2], [1, 0, 2], [2, 2, 0, 1]):
        want = container.pack([dict(entries[b], image_id=k) for k, b in enumerate(picks)])
        _, blob = _prefilled(len(want))
        got = container.pack_groups([comp], [(k, 0, 0, 64, 64, 0, b) for k, b in enumerate(picks)], blob=blob)     # capacity == size: it fits exactly
        assert got.tobytes() == want
    # one batch whose 5 E stream offsets cover all sixteen residues mod 16
    big, want = _batch(kit, RATIOS[0], B=32, seed=3)
    nb = big.nbytes.cpu().numpy().astype(np.int64).reshape(-1)
    offs = 12 + 44 * 32 + np.concatenate([[0], np.cumsum(np.maximum(nb, 0))[:-1]])
    assert set((offs % 16).tolist()) == set(range(16)), "the data set does not start a stream at every residue mod 16"
    assert big.pack(64, 64).tobytes() == want


# ---- 3. ragged groups ----------------------------------------------------------------------------------------------------------
def test_ragged_tiles_interleave_their_groups(kit):
    _, one, many = _ragged(kit)
    assert len(one.groups) == 4 and [t[2:] for t in one.tiles] == [(64, 64), (64, 48), (16, 64), (16, 48)]
    assert container.pack_device(one, first_image_id=7).tobytes() == container.pack(container.entries_from_tiled(one, 7))
    assert one.pack(3).tobytes() == container.pack(container.entries_from_tiled(one, 3))
    # two images from compress_tiled_batch: per image (views of the shared buffers) and as a list (the shared buffers in place)
    per = [container.entries_from_tiled(t, image_id=n) for n, t in enumerate(many)]
    for n, t in enumerate(many):
        assert t.pack(n).tobytes() == container.pack(per[n])
    groups, entries = container._tables_of([many], None, None, 0)
    assert len(groups) == 4 and all(g.data.data_ptr() == w[1].data.data_ptr() and g.batch == 2 * len(w[0]) for g, w in zip(groups, many[0]._whole[0]))
    assert container.pack_device([many]).tobytes() == container.pack(per[0] + per[1]) == container.pack_device(many).tobytes()
    assert len(container._tables_of(many, None, None, 0)[0]) == 4 and len(container._tables_of(many[::-1], None, None, 0)[0]) == 8
    # mixed items: a batch of whole images, then the tiled images, ids counting up
    comp, _ = _batch(kit, RATIOS[1])
    mixed = container.entries_from_batch(comp, 64, 64, 4) + container.entries_from_tiled(many[0], 7) + container.entries_from_tiled(many[1], 8)
    assert container.pack_device([comp, many], 64, 64, first_image_id=4).tobytes() == container.pack(mixed)


# ---- 4. a stream longer than one workgroup's share -------------------------------------------------------------------------------
def test_one_768_tile_as_a_single_entry(kit):
    comp = _compress(kit[1], 1, 768, 768, (0.0, 0.0), 2)          # mode 6: all 36864 indices in the fine stream
    want = container.pack(container.entries_from_batch(comp, 768, 768))
    assert int(comp.nbytes.max()) > 4 * 16 * 256, "the fine stream should span several workgroups of the copy (256 words each)"
    _, blob = _prefilled(len(want) + 64)
    packed = container.pack_device(comp, 768, 768, blob=blob)
    assert packed.tobytes() == want and bool((blob[len(want):] == 0xA5).all())
    back = container.load(want, kit[1], DEV).batch()
    assert back.to_host() == comp.to_host() and torch.equal(back.nbytes, comp.nbytes)


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_reach_python_and_nothing_leaves_the_capacity(kit):
    codec = kit[1]
    comp, want = _batch(kit, RATIOS[0])
    # a symbol outside the table: what to_host() raises
    ind, e16, e8 = _inputs(3, 64, 64, 11)
    ind[1, 0, 0] = 1024                                     # (the top-left cell is coded whichever grain covers it)
    mask, _, _, mode = cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)(torch.from_numpy(e16).to(DEV), torch.from_numpy(e8).to(DEV))
    bad = codec.compress(torch.from_numpy(ind).to(DEV), mask, mode)
    with pytest.raises(KeyError):
        bad.to_host()
    packed = bad.pack(64, 64)
    with pytest.raises(KeyError):
        packed.tobytes()
    with pytest.raises(KeyError):
        packed.nbytes()
    # capacity one byte short: the capacity code, and the bytes behind the blob stay as they were
    buf, blob = _prefilled(len(want) - 1, guard=64)
    packed = container.pack_device(comp, 64, 64, blob=blob)
    with pytest.raises(cg.CgicError) as err:
        packed.tobytes()
    assert err.value.code == cg._lib.ERR_CAPACITY and int(packed.total.cpu()[0]) == cg._lib.ERR_CAPACITY - 10
    assert bool((buf[len(want) - 1:] == 0xA5).all())
    # ... also when the capacity ends inside the headers
    for cap in (11, 12, 100):
        buf, blob = _prefilled(cap, guard=64)
        assert int(container.pack_device(comp, 64, 64, blob=blob).total.cpu()[0]) == cg._lib.ERR_CAPACITY - 10
        assert bool((buf[cap:] == 0xA5).all())
    # the limits: refused before any launch -- `total` keeps its prefill
    torch.cuda.synchronize()
    total = torch.full((1,), -77, dtype=torch.int64, device=DEV)
    _, blob = _prefilled(4096)
    ok = (0, 0, 0, 64, 64, 0, 0)
    for groups, entries in (([comp], [ok, (1, 0, 0, 64, 64, 0, 3)]),            # index >= B_g
                            ([comp], [(0, 0, 0, 64, 64, 0, -1)]),
                            ([comp], [(0, 0, 0, 64, 64, 1, 0)]),                  # a group outside the table
                            ([comp] * 65, [ok]),                                  # G over the limit
                            ([comp], [ok] * 65536)):                              # E over the limit
        with pytest.raises(cg.CgicError) as err:
            container.pack_groups(groups, entries, blob=blob, total=total)
        assert err.value.code == cg._lib.ERR_INVALID
    torch.cuda.synchronize()
    assert int(total.cpu()[0]) == -77 and bool((blob == 0xA5).all())


# ---- 6. load -------------------------------------------------------------------------------------------------------------------
def _same_streams(loaded, blob):
    ref = container.unpack(blob)
    assert sorted(k for idxs, _ in loaded.groups for k in idxs) == list(range(len(ref)))
    for idxs, comp in loaded.groups:
        host = comp.to_host()
        nb = comp.nbytes.cpu().numpy()
        for j, k in enumerate(idxs):
            assert host[j] == ref[k]["streams"] and comp.mode == ref[k]["mode"] and (4 * comp.h, 4 * comp.w) == (ref[k]["height"], ref[k]["width"])
            assert nb[j].tolist() == [len(ref[k]["streams"][n]) if n in ref[k]["streams"] else -1 for n in cg.STREAM_NAMES]


def _same_decode(a, b):
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1])) and torch.equal(a[2], b[2])
    assert int(a[3].abs().max()) == 0 and int(b[3].abs().max()) == 0


@pytest.mark.parametrize("ratio", RATIOS + (EMPTY_COARSE,), ids=lambda r: f"c{r[0]}-m{r[1]}")
def test_load_whole_images_decodes_like_the_original(kit, ratio):
    codec = kit[1]
    comp, blob = _batch(kit, ratio)
    loaded = container.load(blob, codec, DEV, fill=0xFF)            # whatever the slots held before must not matter
    _same_streams(loaded, blob)
    assert loaded.entries["n_entries"] == 3 and loaded.entries["image_id"].tolist() == [0, 1, 2]
    back = loaded.batch()
    assert back is loaded.groups[0][1] and torch.equal(back.nbytes, comp.nbytes) and back.data.shape == comp.data.shape
    # the slack behind every stream is zero up to the end of the 16-byte word that holds byte len + 7
    data, nb = back.data.cpu().numpy(), back.nbytes.cpu().numpy()
    for b in range(3):
        for s in range(5):
            if nb[b, s] >= 0:
                end = ((nb[b, s] + 7) // 16 + 1) * 16
                assert not data[b, s, nb[b, s]:end].any() and (data[b, s, end:] == 0xFF).all()
            else:
                assert (data[b, s] == 0xFF).all()
    for decoder in ("latency", "throughput"):
        _same_decode(codec.decompress(back, decoder=decoder), codec.decompress(comp, decoder=decoder))


def test_load_ragged_tiles_and_decode_them(kit):
    vq, codec = kit
    _, one, many = _ragged(kit)
    blob = container.pack_device([many]).tobytes()
    loaded = container.load(blob, codec, DEV, fill=0xFF)
    _same_streams(loaded, blob)
    # grouped by (height, width, mode) in order of first appearance: the row-major order of the first image's tiles
    assert [(4 * c.h, 4 * c.w, c.batch) for _, c in loaded.groups] == [(64, 64, 2), (64, 48, 2), (16, 64, 2), (16, 48, 2)]
    assert [idxs for idxs, _ in loaded.groups] == [[0, 4], [1, 5], [2, 6], [3, 7]]
    with pytest.raises(ValueError):
        loaded.batch()
    tiled = loaded.tiled((80, 112))
    assert len(tiled) == 2 and all(t.tiles == one.tiles and t.pad == one.pad and t.image_hw == (80, 112) for t in tiled)
    assert [t.streams() for t in tiled] == [t.streams() for t in many]
    # the shared buffers are taken in place
    assert all(t._whole[0] is tiled[0]._whole[0] for t in tiled) and all(w[1] is g[1] for w, g in zip(tiled[0]._whole[0], loaded.groups))
    ref = highres.decompress_tiled_batch(many, codec)
    got = highres.decompress_tiled_batch(tiled, codec)
    for pa, pb in zip(ref, got):
        for (i0, m0, z0), (i1, m1, z1) in zip(pa, pb):
            assert torch.equal(i0, i1) and torch.equal(z0, z1) and all(torch.equal(p, q) for p, q in zip(m0, m1))
    # one image alone, and through decompress_tiled
    alone = container.load(one.pack(5).tobytes(), codec, DEV).tiled((80, 112))
    assert len(alone) == 1 and alone[0].streams() == one.streams()
    per_ref, _ = highres.decompress_tiled(one, codec)
    per_got, _ = highres.decompress_tiled(alone[0], codec)
    for (i0, m0, z0), (i1, m1, z1) in zip(per_ref, per_got):
        assert torch.equal(i0, i1) and torch.equal(z0, z1)
    # a size whose tile grid is not these rectangles
    for hw in ((96, 112), (80, 128), (64, 64)):
        with pytest.raises(ValueError):
            loaded.tiled(hw)
    with pytest.raises(ValueError):
        loaded.tiled((80, 112), tile=48)


def test_load_refuses_on_the_host(kit):
    codec = kit[1]
    fine = dict(image_id=0, y=0, x=0, height=16, width=16, mode=6, streams={"indices_fine": bytes(5000)})
    assert codec.slot_bytes(4, 4) < 5000 + 8
    with pytest.raises(ValueError, match="does not fit the slot"):
        container.load(container.pack([fine]), codec, DEV)
    with pytest.raises(ValueError, match="streams that mode writes"):
        container.load(container.pack([dict(fine, mode=0, streams={"indices_fine": b"ab"})]), codec, DEV)
    with pytest.raises(ValueError, match="multiples of 16"):
        container.load(container.pack([dict(fine, height=20, streams={"indices_fine": b"ab"})]), codec, DEV)
    _, blob = _batch(kit, RATIOS[0])
    for bad in (blob[:-1], blob + b"\0", b"XXXX" + blob[4:]):
        with pytest.raises(ValueError):
            container.load(bad, codec, DEV)
    empty = container.load(container.pack([]), codec, DEV)
    assert empty.groups == [] and empty.entries["n_entries"] == 0


# ---- 7. capture ----------------------------------------------------------------------------------------------------------------
def test_compress_and_pack_captured_and_replayed(kit):
    codec = kit[1]
    B, H, W = 3, 64, 64
    router = cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)

    def host_inputs(seed):
        ind, e16, e8 = _inputs(B, H, W, seed)
        mask, _, _, mode = router(torch.from_numpy(e16).to(DEV), torch.from_numpy(e8).to(DEV))
        return torch.from_numpy(ind).to(DEV), mask, mode

    ind, mask, mode = host_inputs(21)
    step = lambda: container.pack_device(codec.compress(ind, mask, mode), H, W)
    eager = step().tobytes()                                            # one eager call
    assert eager == container.pack(container.entries_from_batch(codec.compress(ind, mask, mode), H, W))
    torch.cuda.synchronize()
    graph, packed = cg.pipeline.capture_graph(step, torch.cuda.Stream())  # (the ticket scope of the other capture tests)
    for seed in (22, 23):
        ind2, mask2, _ = host_inputs(seed)
        ind.copy_(ind2)
        for m, m2 in zip(mask, mask2):
            m.copy_(m2)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = container.pack(container.entries_from_batch(codec.compress(ind2, mask2, mode), H, W))
        assert want != eager and packed.tobytes() == want
    del graph


# ---- 8. the custom op ----------------------------------------------------------------------------------------------------------
def test_custom_op_equals_pack_device(kit):
    comp, want = _batch(kit, RATIOS[0])
    blob, total = torch.ops.cgic.container_pack(comp.data, comp.nbytes, comp.mode, 64, 64, 0)
    slot = comp.data.shape[2]
    assert tuple(blob.shape) == (12 + 44 * 3 + 15 * slot,) == (cg._lib.lib().cgic_container_bound(
        (cg._lib.ContainerGroup * 1)(cg._lib.ContainerGroup(None, None, 3, slot, 0)), 1, 3),)
    assert blob.dtype == torch.uint8 and tuple(total.shape) == (1,) and total.dtype == torch.int64
    assert blob[:int(total)].cpu().numpy().tobytes() == want == container.pack_device(comp, 64, 64).tobytes()
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fb, ft = torch.ops.cgic.container_pack(torch.empty((3, 5, slot), dtype=torch.uint8, device=DEV),
                                               torch.empty((3, 5), dtype=torch.int32, device=DEV), 0, 64, 64, 0)
        assert tuple(fb.shape) == tuple(blob.shape) and fb.dtype == torch.uint8 and tuple(ft.shape) == (1,) and ft.dtype == torch.int64
