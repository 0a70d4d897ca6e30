"""GPU: every decoder path on malformed streams, against the oracle's verdict.

The streams are the catalogue of tests/malformed_ref.py; tests/test_malformed_host.py ties the oracle's verdict on it to the REAL
reference (tests/golden/malformed.npz).  A batch holds mutants at chosen positions -- the first image, the last and one in the middle
are covered in every case -- and clean images elsewhere.  Every comparison is equality:

  clean image                 status 0; indices, masks and z_q exact
  mutant the oracle accepts   status 0; indices, masks and z_q == the oracle's
  mutant the oracle refuses   status != 0
  mutant of the closed list where the library is deliberately stricter than the reference (malformed_ref.STRICTER: a non-canonical
  mask header, a cell both coarse and medium, one symbol broadcast over the cells of a mask)   status != 0

under decoder=None, "latency" and "throughput", with the same status pattern.  ind, the masks, z_q and status are views inside larger
buffers filled with a canary: nothing outside the views changes, and the input bytes and lengths are unchanged after the call.  The
decoder path of every (batch, grid, table, decoder argument) is a row of tests/test_decode_plan_host.py (malformed_ref.GPU_CASES).

No mutant breaks the buffer contract (len + 8 <= slot, the slot zero behind the stream): the tests check verdicts, not crashes.
What bounds the kernels on these inputs, read from the code before the first run (csrc/cgic_decode.hip, cgic_decode_ss.hip):

  reads   every decoder derives the text's end from nbytes and the header byte, clamped at zero (a pad count beyond the payload is an
          empty text); BitWindow / WaveDecoder::fill load 16- / 4-byte words up to nbytes + the slack of the contract and zero the rest;
          a lookup or trie walk stops at `q < nbits` (`rem` in the image decoder, which stages at most its planned stage bytes and
          answers an image whose bits exceed them with "overflow" for its three streams); the merge stages the mask streams word-wise,
          wc + 2 / wm + 2 words of a slot the plan has checked to hold them, whatever their nbytes says.
  writes  a symbol is stored only below the grid's capacity (`put` under `count + rank < cap`, `o < cap`, `n + rank < cap`,
          `at + k < cap_s`); a count beyond it is reported as -3 and never used as an index.  The merge reads coarse and medium symbols at
          ranks below the MASK's popcount (at most the capacity: inside the image's workspace even when the decoded count is smaller),
          fine symbols under `frank < dc_f`, and stages a band only when its three rank ranges fit band_syms.
  exits   in the fused launch every decoder workgroup returns through decode_merge_body, which releases the image's ticket after any
          return of decode_split_body (no stream, `nb <= 0`, more workgroups than parts); a band that refuses a mask header waits for
          the decoders first (wait_decoded) and adds itself to the ticket like every other.  The parts of a split stream are dealt from
          nbytes alone, and each calls part_exchange exactly once, also with an empty text.  The image decoder's sweeps end after at
          most one sweep per chunk."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import long_codes_ref as lc
import malformed_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
gpu = pytest.mark.gpu
GUARD = 64                                  # elements of canary on either side of every output view
DECODERS = (None, "latency", "throughput")


class _V:
    def __init__(self, v): self.v = v
    def item(self): return self.v


def _counts(table):
    from conftest import load_golden
    if table == "zipf":
        return load_golden("coders")["zipf_freq"]
    return np.array(mr.TWO_COUNTS, np.int64) if table == "two" else lc.ladder_table(*table)


@functools.lru_cache(maxsize=None)
def _htab(table):
    from oracle import cgic_oracle as orc
    orc.build()
    t = orc.HuffmanTable(_counts(table))
    assert (t.n, t.maxlen) == mr.table_shape(table)
    return t


@functools.lru_cache(maxsize=None)
def _codec(table, rows=None):
    """(GrainCodec, codebook [rows or K, 4] as numpy)"""
    import control_gic_amd as cg
    counts = _counts(table)
    K = len(counts)
    cbk = np.random.default_rng(K).standard_normal((K, 4)).astype(np.float32)[:rows]
    codec = cg.GrainCodec({str(s): _V(float(counts[s])) for s in lc.push_order(K)}, torch.from_numpy(cbk).to(DEV))
    assert (K, codec.huffman.table.max_len) == mr.table_shape(table)
    return codec, cbk


def _thin(cat):
    """the first and the last mutant of every (class, stream) -- for the grids where a launch holds one image"""
    keep = {}
    for i, m in enumerate(cat):
        keep.setdefault((m.cls, m.kind, m.mode), [i, i])[1] = i
    idx = sorted({i for pair in keep.values() for i in pair})
    return [cat[i] for i in idx]


@functools.lru_cache(maxsize=None)
def _expected(table, h, w):
    """{mode: (clean row, [mutant rows])}, a row = (Mutant, the oracle's (ind, mc, mm, mf) or None, refuse): worked out once per table
    and grid on the CPU and shared by the decoder arguments"""
    from oracle import cgic_oracle as orc
    htab = _htab(table)
    slot = mr.slot_bytes(htab.maxlen, h, w)
    cat = mr.catalogue(orc, htab, h, w, seed=1000 * h + w, slot=slot)
    cat = [m for m in cat if m.cls != "missing"]                      # refused by from_host (tests/test_python_refusals_host.py)
    if h * w > 64 * 64:
        cat = cat[:3] + _thin(cat[3:])
    out = {}
    for m in cat:
        v = mr.verdict(orc, m, htab)
        why = mr.stricter(orc, m, htab)
        row = (m, v, v is None or why is not None)
        if m.cls == "clean":
            assert v is not None and why is None
            out[m.mode] = (row, [])
        else:
            out[m.mode][1].append(row)
    assert sorted(out) == [0, 3, 6]
    return out, slot


def _view(shape, dtype, canary):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, canary):
    return (buf[:GUARD] == canary).all() & (buf[-GUARD:] == canary).all()


def _decompress_into_views(codec, comp, decoder, want_zq=True):
    """cgic_decompress_streams as GrainCodec.decompress issues it, with every output a view inside a canary buffer ->
    (ind, [mc, mm, mf], zq or None, status, guards intact: a 0-d bool tensor on the device)"""
    from control_gic_amd import _lib, codec as cgcodec
    B, h, w = comp.batch, comp.h, comp.w
    bufs = [_view((B, h, w), torch.int64, -77), _view((B, 1, h // 4, w // 4), torch.int32, -77), _view((B, 1, h // 2, w // 2), torch.int32, -77),
            _view((B, 1, h, w), torch.int32, -77), _view((B, 4, h, w), torch.float32, -77.0), _view((B,), torch.int32, -77)]
    (_, ind), (_, mc), (_, mm), (_, mf), (_, zq), (_, status) = bufs
    cbk = codec.codebook.detach().contiguous() if want_zq else None
    ws = torch.empty(_lib.lib().cgic_decompress_workspace_bytes(B, h, w), dtype=torch.uint8, device=DEV)
    with _lib.on_device(comp.data.device):
        _lib.call("cgic_decompress_streams", codec.huffman.table.handle, _lib.ptr(comp.data), comp.data.shape[2], _lib.ptr(comp.nbytes), B, h, w,
                  comp.mode, _lib.ptr(ind), _lib.ptr(mc), _lib.ptr(mm), _lib.ptr(mf), _lib.ptr(cbk), cbk.shape[0] if want_zq else 0,
                  4 if want_zq else 0, _lib.ptr(zq) if want_zq else None, None, None, _lib.ptr(status), _lib.ptr(ws),
                  cgcodec._decoder_flag(decoder), _lib.current_stream(comp.data.device))
    ok = torch.stack([_guards_intact(b, -77) for b, _ in bufs]).all()
    if not want_zq:
        ok = ok & (zq == -77.0).all()
    return ind, [mc, mm, mf], zq if want_zq else None, status, ok


def _positions(B, call):
    """where the mutants of a call sit: all but one image of a batch of 3 (the clean one moves from call to call), three quarters of a
    longer batch with the first, the middle and the last image among them"""
    if B == 1:
        return [0]
    if B == 3:
        return [b for b in range(3) if b != call % 3]
    rest = [b for b in range(B) if b not in (0, B // 2, B - 1)]
    take = rest[call % 4::4]                               # every fourth of the others stays clean
    return sorted(set(range(B)) - set(take))


def _run_mode(codec, cbk, table, B, h, w, slot, clean, rows, want_zq=True, decoders=DECODERS):
    """every mutant row of one mode through as few calls as the batch allows, each call under every decoder argument; one transfer
    to the host per call and decoder.  Returns (the number of (mutant, decoder) verdicts checked, the verdicts that miss): the caller
    asserts that none misses, so that a failure lists every one of the case"""
    import control_gic_amd as cg
    cbk_dev = codec.codebook
    K = cbk.shape[0]
    todo, call, checked, misses = list(rows), 0, 0, []
    covered = set()
    while todo:
        batch = [clean] * B
        for b in _positions(B, call):
            if todo:
                batch[b] = todo.pop(0)
                covered.add(b)
                checked += len(decoders)
        comp = cg.CompressedBatch.from_host([r[0].streams for r in batch], clean[0].mode, h, w, slot, DEV)
        assert comp.data.shape[2] == codec.slot_bytes(h, w)
        data0, nbytes0 = comp.data.clone(), comp.nbytes.clone()
        refuse = [r[2] or (want_zq and r[1] is not None and int(r[1][0].max()) >= K) for r in batch]
        keep = torch.tensor([not r for r in refuse], device=DEV)
        exp = [torch.from_numpy(np.stack([(r[1] if not rf else clean[1])[k] for r, rf in zip(batch, refuse)])).to(DEV) for k in range(4)]
        exp_zq = cbk_dev[exp[0].clamp(0, K - 1)].permute(0, 3, 1, 2) if want_zq else None
        patterns = []
        for decoder in decoders:
            ind, masks, zq, status, guards = _decompress_into_views(codec, comp, decoder, want_zq)
            bad = (ind != exp[0]).flatten(1).any(1)
            for got, want in zip(masks, exp[1:]):
                bad |= (got.flatten(1) != want.flatten(1)).any(1)
            if want_zq:
                bad |= (zq != exp_zq).flatten(1).any(1)
            unchanged = (comp.data == data0).all() & (comp.nbytes == nbytes0).all()
            host = torch.cat([status, (bad & keep).int(), guards.int().view(1), unchanged.int().view(1)]).cpu().tolist()      # the one transfer
            st, wrong, guards_ok, unchanged = host[:B], host[B:2 * B], host[2 * B], host[2 * B + 1]
            where = (mr.gpu_case_id(table, B, h, w), decoder)
            assert guards_ok and unchanged, where + ([r[0].name for r in batch],)
            for b, (r, rf) in enumerate(zip(batch, refuse)):
                if (st[b] != 0) != rf:
                    misses.append(where + (b, r[0].name, "status", st[b], "the oracle refuses" if r[1] is None else
                                           "stricter" if r[2] else "the oracle accepts"))
                elif wrong[b]:
                    misses.append(where + (b, r[0].name, "bits differ from the oracle's"))
            patterns.append([s != 0 for s in st])
        if any(p != patterns[0] for p in patterns):
            misses.append((mr.gpu_case_id(table, B, h, w), "the decoder arguments disagree", [r[0].name for r in batch], patterns))
        call += 1
    if len(rows) >= B:
        assert {0, B // 2, B - 1} <= covered
    return checked, misses


def _ids(cases):
    return [mr.gpu_case_id(*c[:4]) for c in cases]


@gpu
@pytest.mark.parametrize("table,B,h,w,paths", mr.GPU_CASES, ids=_ids(mr.GPU_CASES))
def test_every_path_gives_the_oracles_verdict(table, B, h, w, paths):
    """the catalogue of the grid through the batched decoder, modes 0, 6 and 3, under the three decoder arguments (paths: the plan
    rows of tests/test_decode_plan_host.py)"""
    codec, cbk = _codec(table)
    exp, slot = _expected(table, h, w)
    n, misses = 0, []
    classes = set()
    for mode, (clean, rows) in exp.items():
        checked, missed = _run_mode(codec, cbk, table, B, h, w, slot, clean, rows)
        n, misses = n + checked, misses + missed
        classes |= {r[0].cls for r in rows}
    assert not misses, (len(misses), misses[:12])
    assert {"truncate", "empty", "extend_keep", "extend_adjust", "header", "flip", "overflow", "swap", "length", "mask_header", "noncanonical",
            "one_bit", "two_bits", "overlap"} <= classes
    assert n >= 3 * 60


@gpu
@pytest.mark.parametrize("want_zq", [True, False], ids=["zq", "no_zq"])
def test_index_outside_the_codebook(want_zq):
    """a code table of 1024 symbols with a codebook of 1000 rows: with z_q, an image that holds an index beyond the codebook is
    refused and its neighbour without one is exact; without z_q the library has no codebook to hold the indices to (cgic_hip.h:
    the range of the indices is the gather's check) and returns them as decoded, status 0"""
    import control_gic_amd as cg
    from oracle import cgic_oracle as orc
    codec, cbk = _codec("zipf", rows=1000)
    htab = _htab("zipf")
    h, w = 16, 16
    slot = mr.slot_bytes(htab.maxlen, h, w)
    base = mr.base_images(orc, htab, h, w, seed=5)[0]
    low = base._replace(ind=base.ind % 1000)
    images, exp = [], []
    for b in (base, low, base):
        streams = orc.compress_image(b.ind, *b.masks, b.mode, htab)
        images.append(streams)
        exp.append(orc.decompress_image(streams, b.mode, h, w, htab)[0])
    assert exp[0].max() >= 1000 > exp[1].max()
    with pytest.raises(RuntimeError):
        orc.gather(exp[0], cbk)
    comp = cg.CompressedBatch.from_host(images, base.mode, h, w, slot, DEV)
    for decoder in DECODERS:
        ind, _, zq, status, guards = _decompress_into_views(codec, comp, decoder, want_zq)
        assert bool(guards)
        st = status.cpu().tolist()
        assert [s != 0 for s in st] == ([True, False, True] if want_zq else [False] * 3), (decoder, st)
        for b in range(3):
            if st[b] == 0:
                assert np.array_equal(ind[b].cpu().numpy(), exp[b]), (decoder, b)
        if want_zq:
            assert np.array_equal(zq[1].cpu().numpy(), orc.gather(exp[1], cbk)[0])


@gpu
def test_status_argument_and_views_agree():
    """GrainCodec.decompress with `status=` a view inside a canary buffer == the call with every output a view: same status words,
    same bits for the images that are not flagged, nothing written around the status view"""
    import control_gic_amd as cg
    codec, cbk = _codec("zipf")
    exp, slot = _expected("zipf", 16, 16)
    clean, rows = exp[0]
    batch = [rows[0], clean, rows[len(rows) // 2], rows[-1]]
    comp = cg.CompressedBatch.from_host([r[0].streams for r in batch], 0, 16, 16, slot, DEV)
    for decoder in DECODERS:
        buf, view = _view((4,), torch.int32, -77)
        ind, masks, zq, status = codec.decompress(comp, decoder=decoder, status=view)
        assert status.data_ptr() == view.data_ptr() and bool(_guards_intact(buf, -77))
        ind2, masks2, zq2, status2, _ = _decompress_into_views(codec, comp, decoder)
        assert torch.equal(status, status2) and int(status[1]) == 0
        ok = status == 0
        assert torch.equal(ind[ok], ind2[ok]) and torch.equal(zq[ok], zq2[ok]) and all(torch.equal(a[ok], b[ok]) for a, b in zip(masks, masks2))


@gpu
def test_an_absent_stream_at_the_c_abi():
    """nbytes = -1 on a stream the mode writes, which only a caller of the C ABI can hand over (from_host refuses the dict): an index
    stream is read as an empty file (coarse: all zeros, as the oracle decodes the empty file; fine with fine cells in the mask:
    refused), a mask stream is refused (include/cgic_hip.h)"""
    import control_gic_amd as cg
    from oracle import cgic_oracle as orc
    codec, cbk = _codec("zipf")
    exp, slot = _expected("zipf", 16, 16)
    clean = exp[0][0]
    comp = cg.CompressedBatch.from_host([clean[0].streams] * 4, 0, 16, 16, slot, DEV)
    comp.nbytes[0, 0] = -1                      # indices_coarse
    comp.nbytes[1, 4] = -1                      # mask_medium
    comp.nbytes[2, 2] = -1                      # indices_fine
    want0 = orc.decompress_image(dict(clean[0].streams, indices_coarse=b""), 0, 16, 16, _htab("zipf"))
    assert not np.array_equal(want0[0], clean[1][0]) and (clean[1][3] == 1).any()
    for decoder in DECODERS:
        ind, masks, zq, status, guards = _decompress_into_views(codec, comp, decoder)
        assert bool(guards)
        st = status.cpu().tolist()
        assert [s != 0 for s in st] == [False, True, True, False], (decoder, st)
        assert np.array_equal(ind[0].cpu().numpy(), want0[0]) and np.array_equal(ind[3].cpu().numpy(), clean[1][0]), decoder
        assert all(np.array_equal(m[0, 0].cpu().numpy(), w) for m, w in zip(masks, want0[1:])), decoder
        assert np.array_equal(zq[0].cpu().numpy(), orc.gather(want0[0], cbk)[0]), decoder


# ---------------------------------------------------------------------------- single-stream entry points
@gpu
def test_single_stream_calls_equal_the_reference(golden):
    """HuffmanCoding.decode_bytes / BinaryCoding.decode_bytes == the REAL decompress_string on every single-stream mutant of the
    fixture (None for the empty file)"""
    import control_gic_amd as cg
    g = golden("malformed")
    coders = {"huffman": _codec("zipf")[0].huffman, "binary": cg.BinaryCoding()}
    n = 0
    for i, (name, kind) in enumerate(zip(g["ss_names"].tolist(), g["ss_kind"].tolist())):
        data = g["ss_bytes"][g["ss_bytes_off"][i]:g["ss_bytes_off"][i + 1]].tobytes()
        got = coders[kind].decode_bytes(data)
        if g["ss_none"][i]:
            assert got is None, name
        else:
            assert got == g["ss_syms"][g["ss_syms_off"][i]:g["ss_syms_off"][i + 1]].tolist(), name
        n += 1
    assert n >= 300


@gpu
@pytest.mark.parametrize("table", ["zipf", "two", (1024, 64)], ids=str)
def test_single_stream_call_on_random_bytes(table):
    """seeded random byte strings of 1, 2, 17, 64 and 1500 bytes: decode_bytes == orc.decode"""
    from oracle import cgic_oracle as orc
    huff, htab = _codec(table)[0].huffman, _htab(table)
    for seed in range(4):
        for data in mr.random_bytes(seed):
            want = orc.decode(htab, data)
            assert huff.decode_bytes(data) == want.tolist(), (table, seed, len(data), data[:4])


# ---------------------------------------------------------------------------- container
@gpu
def test_container_gives_the_same_verdict_as_from_host():
    """one refused and one accepted mutant of each stream kind through container.pack -> bytes -> load -> decompress: the same status
    words and, for the images that are not flagged, the same bits as through from_host"""
    import control_gic_amd as cg
    from control_gic_amd import container
    codec, cbk = _codec("zipf")
    h, w = 16, 16
    exp, slot = _expected("zipf", h, w)
    seen = set()
    for mode, (clean, rows) in exp.items():                   # (a container of one mode loads as one batch)
        picked = []
        for kind in mr.INDEX_STREAMS + mr.MASK_STREAMS:
            mine = [r for r in rows if r[0].kind == kind]
            refused = next((r for r in mine if r[1] is None), None)
            accepted = next((r for r in mine if not r[2] and r[0].cls != "empty_valid"), None)
            picked += [r for r in (refused, accepted) if r is not None]
            seen |= {(kind, r is refused) for r in (refused, accepted) if r is not None}
        batch = [clean] + picked
        entries = [dict(image_id=b, y=0, x=0, height=4 * h, width=4 * w, mode=mode, streams=r[0].streams) for b, r in enumerate(batch)]
        blob = container.pack(entries)
        assert container.unpack(blob) == entries
        loaded = container.load(blob, codec, DEV, fill=0).batch()
        direct = cg.CompressedBatch.from_host([r[0].streams for r in batch], mode, h, w, slot, DEV)
        assert torch.equal(loaded.nbytes, direct.nbytes)
        for decoder in DECODERS:
            a = codec.decompress(loaded, decoder=decoder)
            b = codec.decompress(direct, decoder=decoder)
            st = a[3].cpu().tolist()
            assert st == b[3].cpu().tolist() and [s != 0 for s in st] == [r[2] for r in batch], (mode, decoder, st)
            ok = a[3] == 0
            assert torch.equal(a[0][ok], b[0][ok]) and torch.equal(a[2][ok], b[2][ok]) and all(torch.equal(x[ok], y[ok]) for x, y in zip(a[1], b[1]))
            for i in ok.nonzero().flatten().tolist():
                assert np.array_equal(a[0][i].cpu().numpy(), batch[i][1][0]), (mode, decoder, batch[i][0].name)
    assert seen == {(kind, r) for kind in mr.INDEX_STREAMS + mr.MASK_STREAMS for r in (True, False)}
    clean = exp[0][0]
    entries = [dict(image_id=0, y=0, x=0, height=4 * h, width=4 * w, mode=0, streams=clean[0].streams)]
    # a container whose entry lacks a stream of its mode is refused before anything is uploaded, as from_host refuses the dict
    short = dict(entries[0], streams={k: v for k, v in entries[0]["streams"].items() if k != "mask_medium"})
    with pytest.raises(ValueError, match="does not hold the streams that mode writes"):
        container.load(container.pack([short]), codec, DEV)
    with pytest.raises(ValueError, match="stream mask_medium of image 0 is missing"):
        cg.CompressedBatch.from_host([short["streams"]], 0, h, w, slot, DEV)


def test_gpu_cases_name_the_paths_of_the_issue():
    """CPU: the case table reaches every path by name (the plan rows hold each name to the plan header)"""
    paths = {p for c in mr.GPU_CASES for p in c[4]}
    assert paths == {"fused", "image256", "image1024", "split4", "split24", "serial"}
    nodes = int(re.search(r"constexpr\s+int\s+kLdsTrieNodes\s*=\s*(\d+)", open(os.path.join(ROOT, "control-gic_amd", "csrc", "cgic_coder_dev.h")).read()).group(1))
    tables = {c[0] for c in mr.GPU_CASES}
    assert any(isinstance(t, tuple) and t[1] == 64 and t[0] - 1 <= nodes for t in tables), "the trie staged in LDS"
    assert any(isinstance(t, tuple) and t[1] == 64 and t[0] - 1 > nodes for t in tables), "the trie walked in global memory"
    assert any(isinstance(t, tuple) and t[1] == 65 for t in tables) and "two" in tables
    assert any(c[2] * c[3] == 192 * 192 for c in mr.GPU_CASES), "the merge with per-band staging"
