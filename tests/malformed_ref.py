"""Malformed streams for the decoders: a deterministic, seeded catalogue of mutants of valid oracle streams.  Plain numpy and the
CPU oracle; shared by tests/golden/make_golden_malformed.py (which records what the REAL reference makes of every mutant),
tests/test_malformed_host.py and tests/test_malformed_streams.py.

A base image is `orc.compress_image` on a seeded index grid with the oracle router's masks at long_codes_ref.RATIOS (modes 0, 6
and 3).  A mutant is Mutant(name, cls, kind, streams, mode, h, w): `streams` is {stream name: bytes} as CompressedBatch.from_host
takes it, `cls` the mutation class and `kind` the stream it touches.  No mutant breaks the buffer contract: every stream keeps
len + 8 <= slot (slot_bytes restates cgic_compress_slot_bytes; tests/test_malformed_host.py holds it to the library)."""
import collections

import numpy as np

import long_codes_ref as lc

Mutant = collections.namedtuple("Mutant", "name cls kind streams mode h w")
Base = collections.namedtuple("Base", "mode h w ind masks streams syms")
INDEX_STREAMS = ("indices_coarse", "indices_medium", "indices_fine")
MASK_STREAMS = ("mask_coarse", "mask_medium")
EXTEND = (1, 7, 31)
# classes of index-stream mutants whose text is the clean one: the reference decodes them to the clean symbols
TEXT_UNCHANGED = ("extend_adjust",)
# the grids (and seeds) of tests/golden/malformed.npz, under the 1024-symbol Zipf table of golden("coders")
FIXTURE_GRIDS = ((8, 12), (16, 16))
FIXTURE_SEEDS = (812, 1616)


def slot_bytes(max_len, h, w):
    """cgic_compress_slot_bytes: the longest stream of the grid (every code of the longest length), header, pad byte, 8 bytes of
    slack, rounded up to 16"""
    return ((max_len * h * w // 8 + 2 + 8) + 15) // 16 * 16


def base_images(orc, htab, h, w, seed):
    """[Base] at the three ratio pairs: a seeded uniform index grid, the oracle router's masks of seeded entropy maps"""
    rng = np.random.default_rng(seed)
    ind = rng.integers(0, htab.n, (h, w)).astype(np.int64)
    e16, e8 = lc.entropy_maps(1, h, w, seed=seed)
    out = []
    for c, m in lc.RATIOS:
        mc, mm, mf, _, mode = orc.router(e16, e8, c, m, per_image=True, want_gate=False)
        masks = (mc[0, 0], mm[0, 0], mf[0, 0])
        out.append(Base(mode, h, w, ind, masks, orc.compress_image(ind, *masks, mode, htab), orc.select(ind, *masks)))
    assert [b.mode for b in out] == [0, 6, 3]
    return out


def flip(data, payload_bit):
    b = bytearray(data)
    b[1 + (payload_bit >> 3)] ^= 0x80 >> (payload_bit & 7)
    return bytes(b)


def _with_header(data, v):
    return bytes([v]) + data[1:]


def index_mutants(orc, htab, data, syms, slot, seed):
    """[(cls, tag, bytes)] of one valid, non-empty index stream `data` that encodes `syms`"""
    assert len(data) >= 2 and len(syms) >= 1
    lens = np.asarray(htab.len, np.int64)
    starts = lc.start_bits(lens, syms)
    nbits = int(lens[np.asarray(syms)].sum())
    pad = data[0]
    assert (len(data) - 1) * 8 - pad == nbits
    out = [("truncate", "1", data[:-1]), ("truncate", "half", data[:max(1, len(data) // 2)]), ("truncate", "header", data[:1]),
           ("empty", "0", b"")]
    for n in EXTEND:
        if len(data) + n + 8 > slot:
            continue
        for tag, fill in (("00", b"\x00"), ("ff", b"\xff")):
            out.append(("extend_keep", f"{n}x{tag}", data + fill * n))
            if pad + 8 * n <= 255:
                out.append(("extend_adjust", f"{n}x{tag}", _with_header(data + fill * n, pad + 8 * n)))
    last = int(lens[syms[-1]])
    if last >= 2:
        out.append(("cut_codeword", "1", _with_header(data, pad + 1)))                     # the text ends one bit inside the last codeword
    for v in sorted({0, max(pad - 1, 0), pad + 1, 9, 64, 255}):
        if v != pad:
            out.append(("header", str(v), _with_header(data, v)))
    out.append(("header", "over", _with_header(data[:min(len(data), 8)], 255)))            # more pad than the file has payload bits
    out.append(("flip", "first", flip(data, 0)))
    out.append(("flip", "last", flip(data, nbits - 1)))
    for p in (63, 64):
        if p < nbits:
            out.append(("flip", f"b{p}", flip(data, p)))
    blocks = [k for k in range(1, (len(data) + 15) // 16) if 128 * k < nbits]
    for k in blocks[:: max(1, len(blocks) // 6)]:
        out.append(("flip", f"blk{k}", flip(data, 128 * k)))                               # every 16 bytes of stream: one more wave
    deep = np.flatnonzero(lens[np.asarray(syms)] > lc.LUT_BITS)
    if len(deep):
        i = int(deep[len(deep) // 2])
        out.append(("flip", "deep", flip(data, int(starts[i]) + lc.LUT_BITS)))             # inside a codeword, beyond the LUT window
    # flips found on the CPU: some keep the symbol count (accepted, other symbols), some change it (refused)
    rng = np.random.default_rng(seed)
    keep, change = [], []
    for p in rng.permutation(nbits)[:400].tolist():
        n = len(orc.decode(htab, flip(data, p)))
        if n == len(syms) and len(keep) < 3:
            keep.append(p)
        elif n != len(syms) and len(change) < 3:
            change.append(p)
        if len(keep) == 3 and len(change) == 3:
            break
    out += [("flip_keep", f"b{p}", flip(data, p)) for p in keep] + [("flip_change", f"b{p}", flip(data, p)) for p in change]
    short = int(np.argmin(lens))
    n_over = ((slot - 8 - 1) * 8 - 8) // int(lens[short])
    over = orc.encode(htab, np.full(n_over, short, np.int64))
    assert len(over) + 8 <= slot
    out.append(("overflow", "shortest", over))
    seen, uniq = {data}, []
    for cls, tag, d in out:                                                                # (a mutation that gives the clean bytes, or a twin, is dropped)
        assert len(d) + 8 <= slot, (cls, tag)
        if d not in seen:
            seen.add(d)
            uniq.append((cls, tag, d))
    return uniq


def mask_bits(data, n):
    return np.unpackbits(np.frombuffer(data[1:], np.uint8))[:n].astype(np.int32)


def mask_bytes(orc, bits):
    return orc.encode(orc.HuffmanTable.binary(), np.asarray(bits, np.int64))


def mask_mutants(orc, data, n, seed):
    """[(cls, tag, bytes)] of one valid mask stream of n bits; the two-bit and overlap classes need the image (catalogue)"""
    pad = data[0]
    rng = np.random.default_rng(seed)
    return [("length", "short", data[:-1]), ("length", "long", data + b"\x00"), ("length", "empty", b""), ("length", "header", data[:1]),
            ("mask_header", "plus1", _with_header(data, pad + 1)), ("mask_header", "minus1", _with_header(data, pad - 1)),
            ("mask_header", "0", _with_header(data, 0)),
            ("noncanonical", "plus8", _with_header(data + b"\x00", pad + 8)), ("noncanonical", "plus8ff", _with_header(data + b"\xff", pad + 8)),
            ("one_bit", "rnd", flip(data, int(rng.integers(0, n))))]


def _moved_bit(bits, free, rng):
    """bits with one 1 cleared and one 0 (of the positions `free` allows) set, or None"""
    ones, zeros = np.flatnonzero(bits == 1), np.flatnonzero((bits == 0) & free)
    if not len(ones) or not len(zeros):
        return None
    out = bits.copy()
    out[rng.choice(ones)] = 0
    out[rng.choice(zeros)] = 1
    return out


def catalogue(orc, htab, h, w, seed, slot=None):
    """every mutant of the three base images of an h x w grid -> [Mutant]; the first three entries are the clean images"""
    slot = slot_bytes(int(htab.maxlen), h, w) if slot is None else slot
    up = lambda a, k: np.repeat(np.repeat(a, k, -2), k, -1)
    out = []
    bases = base_images(orc, htab, h, w, seed)
    for base in bases:
        out.append(Mutant(f"m{base.mode}-clean", "clean", None, dict(base.streams), base.mode, h, w))
    for bi, base in enumerate(bases):
        mode, st = base.mode, base.streams
        rng = np.random.default_rng(seed + 17 * bi)

        def add(cls, kind, tag, **repl):
            new = dict(st)
            for k, v in repl.items():
                if v is None:
                    del new[k]
                else:
                    new[k] = v
            out.append(Mutant(f"m{mode}-{kind}-{cls}-{tag}", cls, kind, new, mode, h, w))

        for si, name in enumerate(INDEX_STREAMS):
            if name not in st:
                continue
            if not st[name]:                                     # the mask holds no cell of this granularity: an empty file is valid
                add("empty_valid", name, "0", **{name: b""})
                continue
            for cls, tag, d in index_mutants(orc, htab, st[name], base.syms[si], slot, seed + 100 * bi + si):
                add(cls, name, tag, **{name: d})
        if "indices_coarse" in st and st.get("indices_medium"):
            add("swap", "indices_coarse", "medium", indices_coarse=st["indices_medium"], indices_medium=st["indices_coarse"])
        if "indices_coarse" in st and st.get("indices_fine"):
            add("swap", "indices_coarse", "fine", indices_coarse=st["indices_fine"], indices_fine=st["indices_coarse"])
        mc, mm, _ = base.masks
        for name, n in (("mask_coarse", mc.size), ("mask_medium", mm.size)):
            if name not in st:
                continue
            for cls, tag, d in mask_mutants(orc, st[name], n, seed + 100 * bi + 50):
                add(cls, name, tag, **{name: d})
        # two bits, popcount kept, no cell both coarse and medium: the streams are those of the moved mask (another layout, accepted)
        if mode in (0, 3):
            free = (up(mm, 1).reshape(h // 4, 2, w // 4, 2).sum((1, 3)) == 0).ravel() if mode == 0 else np.ones(mc.size, bool)
            moved = _moved_bit(mc.ravel(), free, rng)
            if moved is not None:
                add("two_bits", "mask_coarse", "moved", mask_coarse=mask_bytes(orc, moved))
        if mode == 0:
            moved = _moved_bit(mm.ravel(), up(mc, 2).ravel() == 0, rng)
            if moved is not None:
                add("two_bits", "mask_medium", "moved", mask_medium=mask_bytes(orc, moved))
            # overlap: a medium bit set under a set coarse bit, the medium stream one symbol longer so that the counts match
            under = np.flatnonzero((up(mc, 2).ravel() == 1) & (mm.ravel() == 0))
            if len(under):
                j = int(under[len(under) // 2])
                mm2 = mm.ravel().copy()
                mm2[j] = 1
                rank = int(mm2[:j].sum())
                sym = np.insert(base.syms[1], rank, int(rng.integers(0, htab.n)))
                add("overlap", "mask_medium", f"cell{j}", mask_medium=mask_bytes(orc, mm2), indices_medium=orc.encode(htab, sym))
        for name in st:
            add("missing", name, "absent", **{name: None})
    names = [m.name for m in out]
    assert len(set(names)) == len(names)
    return out


def single_stream_mutants(orc, htab, h, w, seed):
    """the mutants of ONE stream, for the single-stream entry points: [(name, table kind, bytes)] from the catalogue of the grid,
    index streams under the code table, mask streams under the binary one"""
    out, seen = [], set()
    for m in catalogue(orc, htab, h, w, seed):
        if m.kind is None or m.cls in ("missing", "swap", "two_bits", "overlap"):
            continue
        d = m.streams[m.kind]
        kind = "binary" if m.kind in MASK_STREAMS else "huffman"
        if (kind, d) not in seen:
            seen.add((kind, d))
            out.append((m.name, kind, d))
    return out


def random_bytes(seed, sizes=(1, 2, 17, 64, 1500)):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]


def verdict(orc, m, htab):
    """the oracle on a mutant: None if it refuses (raises), else (ind, mask_c, mask_m, mask_f)"""
    try:
        return orc.decompress_image(m.streams, m.mode, m.h, m.w, htab)
    except (RuntimeError, KeyError):
        return None


# ---- where the library is deliberately stricter than the reference ("malformed input"): a closed list
STRICTER = ("noncanonical_mask", "overlap", "one_symbol_broadcast")


def stricter(orc, m, htab):
    """the entry of STRICTER under which the library refuses a mutant that the reference accepts, or None.  Worked out from the
    streams alone, never from what the library answers:
      noncanonical_mask     a mask stream that decodes to the right number of bits but is not 2 + n/8 bytes with pad 8 - n%8
      overlap               mode 0 and a cell both coarse and medium (the reference leaves -1 in the fine mask and in the sum)
      one_symbol_broadcast  an index stream of ONE symbol whose mask holds another number of cells: `t[t == 1] = tensor([s])`
                            broadcasts in the reference"""
    on = orc.mode_streams(m.mode)
    btab = orc.HuffmanTable.binary()
    n = {"mask_coarse": (m.h // 4) * (m.w // 4), "mask_medium": (m.h // 2) * (m.w // 2)}
    bits = {}
    for i, name in ((3, "mask_coarse"), (4, "mask_medium")):
        if on[i] and m.streams.get(name):
            d = m.streams[name]
            dec = orc.decode(btab, d)
            if len(dec) == n[name]:
                bits[name] = dec
                if len(d) != 2 + n[name] // 8 or d[0] != 8 - n[name] % 8:
                    return "noncanonical_mask"
    if m.mode == 0 and len(bits) == 2:
        mc = bits["mask_coarse"].reshape(m.h // 4, m.w // 4)
        mm = bits["mask_medium"].reshape(m.h // 2, m.w // 2)
        if (np.repeat(np.repeat(mc, 2, 0), 2, 1) & mm).any():
            return "overlap"
    v = verdict(orc, m, htab)
    if v is not None and m.mode in (0, 1, 2, 3):
        cells = [int((a == 1).sum()) for a in v[1:]]
        for i in range(3):
            d = m.streams.get(INDEX_STREAMS[i]) if on[i] else None
            if d and len(orc.decode(htab, d)) == 1 and cells[i] != 1:
                return "one_symbol_broadcast"
    return None


# ---- the GPU cases of tests/test_malformed_streams.py and the decoder path each must take (rows of tests/test_decode_plan_host.py):
# (table, B, h, w, (path under auto, latency, throughput)); tables: "zipf" = golden("coders"), "two" = 2 symbols with 1-bit codes,
# (K, L) = the ladder of long_codes_ref with K symbols and a longest code of L bits
TWO_COUNTS = (3, 1)
GPU_CASES = [
    ("zipf", 3, 16, 16, ("fused", "fused", "image256")),
    ("zipf", 3, 64, 64, ("fused", "fused", "image256")),
    ("zipf", 40, 64, 64, ("split4", "split4", "image256")),                 # too many images to fuse
    ("zipf", 1, 192, 192, ("fused", "fused", "image1024")),                 # the merge stages its symbols band by band
    ((1024, 64), 3, 64, 64, ("fused", "fused", "image256")),                # LUT misses walk the trie staged in LDS
    ((1024, 64), 1, 64, 96, ("fused", "fused", "image1024")),
    ((1024, 64), 1, 64, 132, ("fused", "fused", "split24")),
    ((2560, 64), 3, 64, 64, ("fused", "fused", "image256")),                # 2559 trie nodes: walked in global memory
    ((1024, 65), 3, 32, 48, ("serial", "serial", "serial")),
    ("two", 3, 16, 16, ("fused", "fused", "image256")),                     # 1-bit codes: the most symbols per byte
    ("two", 3, 64, 64, ("fused", "fused", "image256")),
]
# (K, longest code) of each table, as the plan sees it
TABLE_SHAPE = {"zipf": (1024, 13), "two": (2, 1)}


def table_shape(table):
    return TABLE_SHAPE.get(table, table)


def gpu_case_id(table, B, h, w):
    k, l = table_shape(table)
    return f"{table if isinstance(table, str) else f'k{k}l{l}'}-{B}x{h}x{w}"
