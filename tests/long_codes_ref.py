"""Code tables with an exact longest code, and index grids that visit their long codes: plain numpy, shared by
tests/golden/make_golden_longcodes.py, tests/test_long_codes_host.py and tests/test_long_codes.py.

ladder_table(K, max_len): counts of K symbols whose Huffman code has lengths 1, 2, ..., D on a ladder of D rungs and the longest
codes, max_len bits, on a body of K - D symbols of count 1 at the ladder's foot.  The rungs grow like Fibonacci numbers, the
slowest growth that still makes every merge of the tree take the running node and the next rung: rung i + 1 is
max(rung i, merged node i - 1) + 1, so when node i - 1 and rung i are merged every later rung is larger than both."""
import heapq

import numpy as np

LUT_BITS = 13                     # kLutBitsMax of csrc/cgic_common.h: codes up to this length resolve in the decoders' LUT
CONTENT = ("uniform", "deepest", "deep_short", "ramp")
# (K, longest code) of the fixture tests/golden/long_codes.npz
FIXTURE_TABLES = ((1024, 14), (1024, 32), (1024, 33), (1024, 63), (1024, 64), (1024, 65), (2560, 64))


def push_order(n):
    """the order in which the reference's counter (a ParameterDict keyed str(i)) hands its entries to the heap: keys as strings"""
    return sorted(range(n), key=str)


class _Node:
    __slots__ = ("freq", "sym", "left", "right")

    def __init__(self, freq, sym=None, left=None, right=None):
        self.freq, self.sym, self.left, self.right = freq, sym, left, right

    def __lt__(self, other):          # ties are left to the heap's own order, as a comparison on the count alone leaves them
        return self.freq < other.freq


def huffman_lengths(counts, order=None):
    """code lengths of the Huffman tree built with a binary heap compared on the counts alone, leaves pushed in `order`"""
    counts = [int(v) for v in counts]
    heap = []
    for s in (push_order(len(counts)) if order is None else order):
        heapq.heappush(heap, _Node(counts[s], s))
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        heapq.heappush(heap, _Node(a.freq + b.freq, None, a, b))
    lens = np.zeros(len(counts), np.int32)
    stack = [(heap[0], 0)]
    while stack:
        node, depth = stack.pop()
        if node.sym is not None:
            lens[node.sym] = depth
        else:
            stack.append((node.right, depth + 1))
            stack.append((node.left, depth + 1))
    return lens


def _ladder_counts(K, D):
    """symbols 0 .. K-D-1: the body of ones; symbol K-D+i: rung i (i = 0 is the lowest: the longest ladder code, D bits)"""
    body = K - D
    counts = np.ones(K, np.int64)
    rung, merged_before, merged = 1, 0, body          # the body's root plays merged node 0; no rung and no node before it
    for i in range(D):
        rung = max(rung, merged_before) + 1 if i else body + 1
        counts[body + i] = rung
        merged_before, merged = merged, merged + rung
    return counts


def ladder_table(K, max_len, lengths=huffman_lengths):
    """int64 counts [K] whose code table has the longest code max_len: the number of rungs D is searched, and the longest code of
    the table found is asserted with `lengths` (counts -> code lengths), never assumed.  Every count stays below 2^53."""
    for D in range(max(1, max_len - 2 * K.bit_length()), min(max_len, K - 1)):
        counts = _ladder_counts(K, D)
        assert int(counts.max()) < 2 ** 53 and int(counts.sum()) < 2 ** 53, (K, max_len, D)
        ln = lengths(counts)
        if int(ln.max()) == max_len:
            body = K - D
            assert [int(v) for v in ln[body:]] == list(range(D, 0, -1)), "the rungs carry lengths D .. 1"
            assert int(ln[:body].min()) >= D, "the body lies below the ladder"
            return counts
    raise AssertionError(f"no ladder of {K} symbols has a longest code of {max_len} bits")


def content_grid(kind, lens, shape, rng=None):
    """index grid of `shape` (any number of axes) of one content class, built from the table's own code lengths `lens`:
    uniform     every symbol, shuffled (nearly all codewords have the longest length)
    deepest     one symbol of the longest length, repeated
    deep_short  that symbol and the 1-bit symbol, alternating: boundaries advance by max_len + 1 bits
    ramp        one symbol per code length that the table has, in order of length, cyclic"""
    lens = np.asarray(lens)
    n = int(np.prod(shape))
    deep = int(np.flatnonzero(lens == lens.max())[0])
    if kind == "uniform":
        reps = -(-n // len(lens))
        flat = np.tile(np.arange(len(lens)), reps)
        (rng or np.random.default_rng(len(lens) + n)).shuffle(flat)
        flat = flat[:n]
    elif kind == "deepest":
        flat = np.full(n, deep)
    elif kind == "deep_short":
        short = int(np.flatnonzero(lens == lens.min())[0])
        assert lens[short] == 1
        flat = np.where(np.arange(n) % 2 == 0, deep, short)
    elif kind == "ramp":
        flat = np.resize(ramp_symbols(lens), n)
    else:
        raise ValueError(kind)
    return flat.astype(np.int64).reshape(shape)


def ramp_symbols(lens, only=None):
    """the first symbol of every code length the table has (of the lengths in `only`, if given), by ascending length"""
    lens = np.asarray(lens)
    return np.array([int(np.flatnonzero(lens == v)[0]) for v in sorted(set(lens.tolist())) if only is None or v in only], np.int64)


def named_lengths(lens):
    """the lengths the non-vacuity rule names, as far as the table has them: lut_bits + 1, 32, 33 and the longest"""
    have = set(np.asarray(lens).tolist())
    return [v for v in sorted({LUT_BITS + 1, 32, 33, int(max(have))}) if v in have]


def start_bits(lens, syms):
    """bit offset in the stream's payload at which each codeword of `syms` starts (the payload follows the one header byte)"""
    ln = np.asarray(lens, np.int64)[np.asarray(syms, np.int64).ravel()]
    return np.concatenate([[0], np.cumsum(ln)[:-1]]) if len(ln) else np.zeros(0, np.int64)


def fixture_streams(lens):
    """the symbol streams tests/golden/long_codes.npz records for a table: none, 1 and 2 symbols, 65 symbols, and 1024 symbols of
    every content class -> [(name, int64 symbols)]"""
    out = [("n0", np.zeros(0, np.int64)), ("n1", content_grid("deepest", lens, (1,))), ("n2", content_grid("deep_short", lens, (2,))),
           ("n65", content_grid("ramp", lens, (65,)))]
    return out + [(kind, content_grid(kind, lens, (1024,))) for kind in CONTENT]


# ---- the cases of the batched codec (tests/test_long_codes.py) and the decoder path each must take (tests/test_decode_plan_host.py)
RATIOS = ((0.1, 0.8), (0.0, 0.0), (0.5, 0.5))
DECODERS = ("auto", "latency", "throughput")
# (K, longest code, B, h, w) -> the path of cgic_decode_plan.h at 256 CUs under (auto, latency, throughput), worked out by hand:
# a launch fuses while B x (decoder workgroups 4 | 16 beyond 64x64 + merge bands) <= 128 CUs (256 under "latency"); "throughput"
# takes the self-synchronising image decoder while 4 x 2^13 + 21/16 h w x max_len x 11/64 bytes (about) stay within 150 KB, with
# 256 threads up to 64x64 and 1024 beyond; what neither takes goes to the split decoder (4 | 24 workgroups per image), and a code
# beyond 64 bits to the serial one
_TINY = {L: [(1, 4, 4, ("fused", "fused", "image256")), (1, 8, 12, ("fused", "fused", "image256")),
             (3, 64, 64, ("fused", "fused", "image256"))] for L in (14, 32, 33, 63, 64)}
CODEC_CASES = []
for _L, _rows in _TINY.items():
    CODEC_CASES += [(1024, _L) + r for r in _rows]
    # 96x96: the image decoder's LDS fits up to 33 bits (large workgroup); at 63 and 64 bits "throughput" falls back to the split one
    CODEC_CASES.append((1024, _L, 1, 96, 96, ("fused", "fused", "image1024" if _L <= 33 else "split24")))
CODEC_CASES += [
    (1024, 33, 40, 64, 64, ("split4", "split4", "image256")),
    (1024, 64, 40, 64, 64, ("split4", "split4", "image256")),
    # 12 x (16 + 4 bands) = 240 workgroups: fused only when the call has the chip to itself
    (1024, 64, 12, 96, 96, ("split24", "fused", "split24")),
    (1024, 64, 2, 128, 128, ("fused", "fused", "split24")),
    # the largest grid whose image decoder fits at 64 bits (522 coarse cells: 153 568 of 153 600 bytes): the large workgroup
    (1024, 63, 1, 72, 116, ("fused", "fused", "image1024")),
    (1024, 64, 1, 72, 116, ("fused", "fused", "image1024")),
    (1024, 65, 3, 32, 48, ("serial", "serial", "serial")),
    (1024, 65, 1, 64, 64, ("serial", "serial", "serial")),
    (2560, 64, 3, 64, 64, ("fused", "fused", "image256")),
    (96, 33, 3, 32, 48, ("fused", "fused", "image256")),
]
# the forms of the encoder that cgic_coder_plan.h distinguishes, with the 64-bit table of 1024 symbols, at the smallest grid (and
# batch) that reaches each: (form, B, h, w, decoder paths)
FORM_CASES = [
    ("lds-small", 1, 64, 64, ("fused", "fused", "image256")),          # up to kLdsPosSmall positions: the small instantiation
    ("lds", 1, 64, 96, ("fused", "fused", "image1024")),               # up to kLdsPos positions: phase-A results stay in LDS
    ("parts", 1, 64, 132, ("fused", "fused", "split24")),              # beyond kLdsPos: the fine stream in 3 parts, each staged
    ("staged", 683, 64, 132, ("split24", "split24", "split24")),       # 6 B beyond one ticket request: unsplit, the whole stream staged
    ("global", 1, 588, 588, ("fused", "fused", "split24")),            # a part beyond kEncStageMax: unsplit, through the workspace
]


def case_id(K, L, B, h, w):
    return f"k{K}-l{L}-{B}x{h}x{w}"


def merged_grid(ind, mc, mm, mf):
    """what decoding gives back: every position carries the index of the top-left element of the cell of its granularity"""
    up = lambda a, k: np.repeat(np.repeat(a, k, -2), k, -1)
    out = np.where(mf == 1, ind, 0)
    out = out + up(np.where(mm == 1, ind[..., ::2, ::2], 0), 2)
    return out + up(np.where(mc == 1, ind[..., ::4, ::4], 0), 4)


def entropy_maps(B, h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((B, h // 4, w // 4)) * 2.6).astype(np.float32), (rng.random((B, h // 2, w // 2)) * 2.6).astype(np.float32)


def grid_contents(lens, B, h, w):
    """{class: index grid [B, h, w]} for one case.  ramp: cyclic over every length of the table; a grid with fewer positions than
    the table has lengths takes the lengths the non-vacuity rule names, and a grid that cannot hold even those has no ramp"""
    out = {k: content_grid(k, lens, (B, h, w)) for k in CONTENT if k != "ramp"}
    ramp = ramp_symbols(lens)
    if len(ramp) > h * w:
        ramp = ramp_symbols(lens, only=named_lengths(lens))
    if len(ramp) <= h * w:
        out["ramp"] = np.resize(ramp, B * h * w).reshape(B, h, w).astype(np.int64)
    return out


def checked_images(B):
    return list(range(B)) if B <= 3 else [0, B // 2, B - 1]
