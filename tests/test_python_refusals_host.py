"""CPU: what the Python layer refuses, for both sides of every entry point that is bound once and reached twice (a class method
and its torch.ops.cgic op; model.decoder_blend_* with and without `out=`), and the schema of every op.

The calls run under FakeTensorMode on fake "cuda" tensors: every check below sits in front of the first data_ptr(), so no device
is needed and no kernel runs.  An op is called through its Python implementation (under the mode the dispatcher would take the
op's fake kernel, which checks nothing).  One row = (call, exception type, the full message); the messages and the schema strings
were recorded before the bindings were merged, and the table passes unchanged after."""
import functools

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import control_gic_amd as cg
from control_gic_amd import codec as cgcodec, model as cgmodel, ops, pipeline, quantize, rate

f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8

CPU_TENSOR = ("control_gic_amd ops run on an MI355X (HIP) device only; got a CPU tensor. "
              "There is deliberately no CPU fallback -- the CPU oracle lives in oracle/ and is test-only.")
NULL_TABLE = "cgic ops: the code table handle is NULL (pass HuffmanCoding(...).table.handle.value)"
INT32_MASKS = "masks must be int32 like the router's (RouterTriple.py:92)"
IND = "ind must be int64 with B*h*w elements"
BLEND_M_OP = "decoder_blend_medium: h, h_medium on the medium grid; mask_c at half of it, mask_m on it"
BLEND_M_OUT = "decoder_blend_medium: h, h_medium on the medium grid; mask[0] at half of it, mask[1] on it"
BLEND_F = "decoder_blend_fine: h, h_fine on the fine grid; masks at 1/4, 1/2, 1/1 of it"
DECODERS = "['auto', 'latency', 'throughput']"

B, H, W = 2, 16, 24                     # the latent grid of a 64x96 image


@functools.lru_cache(maxsize=None)
def _coder():
    """one real code table for all rows (built outside the fake mode: the table is host-side state of the library)"""
    return cg.HuffmanCoding({str(i): torch.tensor([float(1 + i)]) for i in range(16)})


def _handle():
    return _coder().table.handle.value


def T(*shape, dtype=f32, device="cuda"):
    return torch.empty(shape, dtype=dtype, device=device)


def masks(dtype=i32, h=H, w=W, device="cuda"):
    return [T(B, 1, h // 4, w // 4, dtype=dtype, device=device), T(B, 1, h // 2, w // 2, dtype=dtype, device=device),
            T(B, 1, h, w, dtype=dtype, device=device)]


def impl(op):
    """the Python implementation behind a torch.library custom op"""
    return op._init_fn


def _gc(codebook=True):
    return cg.GrainCodec(_coder(), T(16, 4) if codebook else None)


def _comp(device="cuda"):
    slot = cgcodec.GrainCodec(_coder()).slot_bytes(H, W)
    return cg.CompressedBatch(T(B, 5, slot, dtype=u8, device=device), T(B, 5, dtype=i32, device=device), 0, H, W)


def _direct(monkeypatch, name):
    """torch.ops.cgic.<name> -> the op's Python implementation: how a caller that goes through the dispatcher (model.* without
    `out=`) reaches the checks under the fake mode"""
    monkeypatch.setattr(torch.ops.cgic, name, impl(getattr(ops, name)))


# ---- (id, call, exception type, message); every call runs inside the fake mode
def _compress_rows():
    cls = lambda ind, m, **kw: _gc().compress(ind, m, 0, **kw)
    op = lambda ind, m, table=None: impl(ops.compress_streams)(ind, m[0], m[1], m[2], 0, _handle() if table is None else table, None)
    rows = []
    for side, call in (("GrainCodec.compress", cls), ("ops.compress_streams", op)):
        rows += [(f"{side}: int32 ind", lambda call=call: call(T(B, H, W, dtype=i32), masks()), ValueError, IND),
                 (f"{side}: ind of another grid", lambda call=call: call(T(B, H, W + 1, dtype=i64), masks()), ValueError, IND),
                 (f"{side}: float masks", lambda call=call: call(T(B, H, W, dtype=i64), masks(f32)), TypeError, INT32_MASKS),
                 (f"{side}: one float mask", lambda call=call: call(T(B, H, W, dtype=i64), masks()[:2] + [T(B, 1, H, W)]), TypeError, INT32_MASKS),
                 (f"{side}: CPU ind", lambda call=call: call(T(B, H, W, dtype=i64, device="cpu"), masks()), RuntimeError, CPU_TENSOR),
                 (f"{side}: CPU masks", lambda call=call: call(T(B, H, W, dtype=i64), masks(device="cpu")), RuntimeError, CPU_TENSOR)]
    rows.append(("ops.compress_streams: NULL table", lambda: op(T(B, H, W, dtype=i64), masks(), table=0), ValueError, NULL_TABLE))
    return rows


def _decompress_rows():
    op = lambda decoder="auto", table=None, device="cuda": impl(ops.decompress_streams)(
        _comp(device).data, _comp(device).nbytes, H, W, 0, _handle() if table is None else table, T(16, 4), decoder)
    status = "status must be a contiguous int32 tensor with one element per image on the streams' device"
    return [
        ("GrainCodec.decompress: no codebook", lambda: _gc(False).decompress(_comp()), ValueError, "GrainCodec was built without a codebook"),
        ("GrainCodec.decompress: post_quant_conv without z_q",
         lambda: _gc(False).decompress(_comp(), want_zq=False, post_quant_conv=(T(4, 4), T(4))), ValueError, "post_quant_conv needs want_zq"),
        ("GrainCodec.decompress: int64 status", lambda: _gc().decompress(_comp(), status=T(B, dtype=i64)), ValueError, status),
        ("GrainCodec.decompress: short status", lambda: _gc().decompress(_comp(), status=T(B - 1, dtype=i32)), ValueError, status),
        ("GrainCodec.decompress: strided status", lambda: _gc().decompress(_comp(), status=T(B, 2, dtype=i32)[:, 0]), ValueError, status),
        ("GrainCodec.decompress: CPU status", lambda: _gc().decompress(_comp(), status=T(B, dtype=i32, device="cpu")), ValueError, status),
        ("decoder_mode: unknown name", lambda: cg.decoder_mode("fast"), ValueError, f"decoder mode 'fast': expected one of {DECODERS}"),
        ("the decoder of a call: unknown name", lambda: cgcodec._decoder_flag("fast"), ValueError,
         f"decoder mode 'fast': expected one of {DECODERS}"),
        ("ops.decompress_streams: unknown decoder", lambda: op("fast"), ValueError, f"decoder 'fast': expected one of {DECODERS}"),
        ("ops.decompress_streams: CPU streams", lambda: op(device="cpu"), RuntimeError, CPU_TENSOR),
        # mode 3 writes the coarse and the medium indices and the coarse mask: image 1 lacks one of them (the reference: FileNotFoundError)
        ("CompressedBatch.from_host: a stream of the mode is missing",
         lambda: cg.CompressedBatch.from_host([{"indices_coarse": b"", "indices_medium": b"", "mask_coarse": b""},
                                               {"indices_coarse": b"", "mask_coarse": b"", "indices_fine": b""}], 3, H, W, 4096, "cuda"),
         ValueError, "stream indices_medium of image 1 is missing: mode 3 writes it"),
    ]


def _stream_rows():
    enc, dec = impl(ops.encode_stream), impl(ops.decode_stream)
    short = "decode_stream: uint8 buffer of at least nbytes + 16 bytes"
    return [
        ("HuffmanCoding.encode_to_bytes: CPU symbols", lambda: _coder().encode_to_bytes(T(100, dtype=i64, device="cpu")), RuntimeError, CPU_TENSOR),
        ("BinaryCoding.encode_to_bytes: CPU bits", lambda: cg.BinaryCoding().encode_to_bytes(T(100, dtype=i32, device="cpu")), RuntimeError, CPU_TENSOR),
        ("ops.encode_stream: float symbols", lambda: enc(T(100), _handle()), TypeError, "encode_stream: int64 / int32 symbols"),
        ("ops.encode_stream: no symbols", lambda: enc(T(0, dtype=i64), _handle()), ValueError,
         "encode_stream: an empty input is an empty FILE in the reference (indices_coding.py:116-118), not a stream"),
        ("ops.encode_stream: CPU symbols", lambda: enc(T(100, dtype=i64, device="cpu"), _handle()), RuntimeError, CPU_TENSOR),
        ("ops.encode_stream: NULL table", lambda: enc(T(100, dtype=i64), 0), ValueError, NULL_TABLE),
        ("ops.decode_stream: int32 buffer", lambda: dec(T(64, dtype=i32), 20, _handle()), ValueError, short),
        ("ops.decode_stream: buffer without the 16 bytes of slack", lambda: dec(T(35, dtype=u8), 20, _handle()), ValueError, short),
        ("ops.decode_stream: CPU buffer", lambda: dec(T(64, dtype=u8, device="cpu"), 20, _handle()), RuntimeError, CPU_TENSOR),
    ]


def _blend_rows():
    C = 8
    h = lambda *hw, device="cuda": T(B, C, *hw, device=device)
    m2 = lambda dtype=i32: masks(dtype)[1:]                                      # the medium blend: masks at 1/2 and 1/1 of ITS grid
    rows = []
    # decoder_blend_medium(h, h_medium, mask_c, mask_m) on the grid H x W; the three ways in, each with its own shape refusal
    ways = (("ops.decoder_blend_medium", lambda a, b, m: impl(ops.decoder_blend_medium)(a, b, m[0], m[1]), BLEND_M_OP),
            ("model.decoder_blend_medium(out=)", lambda a, b, m: cgmodel.decoder_blend_medium(a, b, m, out=a), BLEND_M_OUT))
    for side, call, text in ways:
        rows += [(f"{side}: float masks", lambda call=call: call(h(H, W), h(H, W), m2(f32)), TypeError, INT32_MASKS),
                 (f"{side}: h_medium on another grid", lambda call=call: call(h(H, W), h(H, W + 2), m2()), ValueError, text),
                 (f"{side}: mask_c on the full grid", lambda call=call: call(h(H, W), h(H, W), [m2()[1], m2()[1]]), ValueError, text),
                 (f"{side}: mask_m at half the grid", lambda call=call: call(h(H, W), h(H, W), [m2()[0], m2()[0]]), ValueError, text),
                 (f"{side}: CPU h", lambda call=call: call(h(H, W, device="cpu"), h(H, W), m2()), RuntimeError, CPU_TENSOR)]
    ways = (("ops.decoder_blend_fine", lambda a, b, m: impl(ops.decoder_blend_fine)(a, b, *m)),
            ("model.decoder_blend_fine(out=)", lambda a, b, m: cgmodel.decoder_blend_fine(a, b, m, out=a)))
    for side, call in ways:
        rows += [(f"{side}: float masks", lambda call=call: call(h(H, W), h(H, W), masks(f32)), TypeError, INT32_MASKS),
                 (f"{side}: h_fine on another grid", lambda call=call: call(h(H, W), h(H + 4, W), masks()), ValueError, BLEND_F),
                 (f"{side}: masks of another grid", lambda call=call: call(h(H, W), h(H, W), masks(h=H + 4)), ValueError, BLEND_F),
                 (f"{side}: mask_m at a quarter", lambda call=call: call(h(H, W), h(H, W), [masks()[0], masks()[0], masks()[2]]), ValueError, BLEND_F),
                 (f"{side}: CPU masks", lambda call=call: call(h(H, W), h(H, W), masks(device="cpu")), RuntimeError, CPU_TENSOR)]
    gm = impl(ops.grain_merge)
    rows += [
        ("ops.grain_merge: float masks", lambda: gm(h(H // 4, W // 4), h(H // 2, W // 2), h(H, W), *masks(f32)), TypeError, INT32_MASKS),
        ("ops.grain_merge: h_medium on the fine grid", lambda: gm(h(H // 4, W // 4), h(H, W), h(H, W), *masks()), ValueError,
         "h_coarse / h_medium must be the fine map's shape divided by 4 / 2"),
        ("ops.grain_merge: masks of another grid", lambda: gm(h(H // 4, W // 4), h(H // 2, W // 2), h(H, W), *masks(h=H + 4)), ValueError,
         "grain_merge: masks at 1/4, 1/2, 1/1 of the fine grid, one per image"),
        ("ops.grain_merge: CPU h_fine", lambda: gm(h(H // 4, W // 4), h(H // 2, W // 2), h(H, W, device="cpu"), *masks()), RuntimeError, CPU_TENSOR),
        ("ops.avg_pool: CPU x", lambda: impl(ops.avg_pool)(h(H, W, device="cpu"), 2), RuntimeError, CPU_TENSOR),
        ("ops.index_histogram: int32 indices", lambda: impl(ops.index_histogram)(T(100, dtype=i32), T(16, dtype=i64)), TypeError,
         "index_histogram: int64 indices and histogram"),
        ("ops.index_histogram: float histogram", lambda: impl(ops.index_histogram)(T(100, dtype=i64), T(16)), TypeError,
         "index_histogram: int64 indices and histogram"),
        ("ops.index_histogram: CPU histogram", lambda: impl(ops.index_histogram)(T(100, dtype=i64), T(16, dtype=i64, device="cpu")),
         RuntimeError, CPU_TENSOR),
    ]
    return rows


def _rate_rows():
    h16, w16 = H // 4, W // 4
    inds = lambda: [T(B, h16, w16, dtype=i64), T(B, 2 * h16, 2 * w16, dtype=i64), T(B, H, W, dtype=i64)]
    e16, e8, bad8 = lambda: T(B, h16, w16), lambda: T(B, 2 * h16, 2 * w16), lambda: T(B, 3, 3)
    e8_text = f"e8 (2, 3, 3) must be [B, 2*h16, 2*w16] of (2, {h16}, {w16})"
    budget = lambda: T(1, dtype=i64)
    return [
        ("ops.rate_curve: NULL table", lambda: impl(ops.rate_curve)(*inds(), e16(), e8(), 0.1, 0), ValueError, NULL_TABLE),
        ("ops.rate_table: NULL table", lambda: impl(ops.rate_table)(*inds(), e16(), e8(), [0.1], [0.5], True, 0), ValueError, NULL_TABLE),
        ("ops.route_to_bpp: NULL table", lambda: impl(ops.route_to_bpp)(*inds(), e16(), e8(), 0.1, budget(), 0), ValueError, NULL_TABLE),
        ("ops.rate_table: ratio lists of two lengths", lambda: impl(ops.rate_table)(*inds(), e16(), e8(), [0.1, 0.2], [0.5], True, _handle()),
         ValueError, "rate_table: one medium ratio per coarse ratio"),
        # the codec and the raw handle reach the same input checks
        ("rate.rate_curve(codec): e8 of another grid", lambda: rate.rate_curve(_gc(), *inds(), e16(), bad8(), 0.1), ValueError, e8_text),
        ("ops.rate_curve(handle): e8 of another grid", lambda: impl(ops.rate_curve)(*inds(), e16(), bad8(), 0.1, _handle()), ValueError, e8_text),
        ("rate.rate_table(codec): e8 of another grid", lambda: rate.rate_table(_gc(), *inds(), e16(), bad8(), [(0.1, 0.5)]), ValueError, e8_text),
        ("ops.rate_table(handle): e8 of another grid", lambda: impl(ops.rate_table)(*inds(), e16(), bad8(), [0.1], [0.5], True, _handle()),
         ValueError, e8_text),
        ("rate.route_to_bpp(codec): e8 of another grid", lambda: rate.route_to_bpp(_gc(), *inds(), e16(), bad8(), 0.1, target_bpp=1.0),
         ValueError, e8_text),
        ("ops.route_to_bpp(handle): e8 of another grid", lambda: impl(ops.route_to_bpp)(*inds(), e16(), bad8(), 0.1, budget(), _handle()),
         ValueError, e8_text),
        ("rate.route_to_bpp: target and budget", lambda: rate.route_to_bpp(_gc(), *inds(), e16(), e8(), 0.1, target_bpp=1.0, budget=budget()),
         ValueError, "route_to_bpp: give target_bpp or budget (one of them)"),
        ("rate.rate_curve_tiled: no group", lambda: rate.rate_curve_tiled(_gc(), [], 0.1), ValueError, "rate_curve_tiled: no tile group"),
        ("rate.gather_grain_indices: float masks", lambda: rate.gather_grain_indices(*inds(), masks(f32)), TypeError,
         "masks must be int32 like the router's"),
        ("ops.gather_grain_indices: float masks", lambda: impl(ops.gather_grain_indices)(*inds(), *masks(f32)), TypeError,
         "masks must be int32 like the router's"),
        ("rate.gather_grain_indices: masks of another grid", lambda: rate.gather_grain_indices(*inds(), [masks()[1], masks()[1], masks()[2]]),
         ValueError, "masks at 1/4, 1/2, 1/1 of the fine grid expected"),
    ]


def _routing_rows():
    h16, w16 = H // 4, W // 4
    router = lambda: cg.TripleGrainFixedEntropyRouter(0.1, 0.8, per_image=True)
    return [
        ("router: e8 of another grid", lambda: router()(T(B, h16, w16), T(B, 3, 3)), ValueError,
         f"x_entropy_p8 (2, 3, 3) must be [B, 2*h16, 2*w16] of (2, {h16}, {w16})"),
        ("router: CPU maps", lambda: router()(T(B, h16, w16, device="cpu"), T(B, 2 * h16, 2 * w16)), RuntimeError, CPU_TENSOR),
        ("vq_forward_route: maps of another batch", lambda: quantize.vq_forward_route(T(B, 4, H, W), T(16, 4), 0.25, True, T(B + 1, h16, w16),
                                                                                       T(B + 1, 2 * h16, 2 * w16), 0.1, 0.8), ValueError,
         "entropy maps do not match the latent batch"),
        ("vq_forward_route: e8 of another grid", lambda: quantize.vq_forward_route(T(B, 4, H, W), T(16, 4), 0.25, True, T(B, h16, w16), T(B, 3, 3),
                                                                                    0.1, 0.8, pixels=T(B, 3, 4 * H, 4 * W)), ValueError,
         "entropy maps do not match the latent batch"),
        ("HotCall: an image that is no multiple of 16", lambda: pipeline.HotCall(None, 0.1, 0.8, B, 64, 100), ValueError,
         "H and W must be multiples of 16"),
    ]


ROWS = _compress_rows() + _decompress_rows() + _stream_rows() + _blend_rows() + _rate_rows() + _routing_rows()


@pytest.mark.parametrize("call, exc, message", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_refusal(call, exc, message):
    _coder()
    with FakeTensorMode():
        with pytest.raises(exc) as got:
            call()
    assert type(got.value) is exc
    assert got.value.args[0] == message


@pytest.mark.parametrize("name, call, exc, message", [
    ("decoder_blend_medium", lambda m: cgmodel.decoder_blend_medium(T(B, 8, H, W), T(B, 8, H, W + 2), m[1:]), ValueError, BLEND_M_OP),
    ("decoder_blend_medium", lambda m: cgmodel.decoder_blend_medium(T(B, 8, H, W), T(B, 8, H, W), [m[1].float(), m[2]]), TypeError, INT32_MASKS),
    ("decoder_blend_fine", lambda m: cgmodel.decoder_blend_fine(T(B, 8, H, W), T(B, 8, H + 4, W), m), ValueError, BLEND_F),
    ("decoder_blend_fine", lambda m: cgmodel.decoder_blend_fine(T(B, 8, H, W), T(B, 8, H, W), [m[0], m[1], m[2].float()]), TypeError, INT32_MASKS),
    ("grain_merge", lambda m: cgmodel.grain_merge(T(B, 8, H // 4, W // 4), T(B, 8, H, W), T(B, 8, H, W), m), ValueError,
     "h_coarse / h_medium must be the fine map's shape divided by 4 / 2"),
])
def test_refusal_of_the_model_functions_without_out(monkeypatch, name, call, exc, message):
    """model.decoder_blend_* without `out=` (and model.grain_merge) go through the op: the op's refusal, the op's text"""
    _direct(monkeypatch, name)
    with FakeTensorMode():
        with pytest.raises(exc) as got:
            call(masks())
    assert type(got.value) is exc and got.value.args[0] == message


def test_an_empty_input_is_an_empty_file_for_the_coder_and_an_error_for_the_op():
    huff, binary = _coder(), cg.BinaryCoding()
    with FakeTensorMode():
        assert huff.encode_to_bytes(T(0, dtype=i64)) == b""
        assert huff.encode_to_bytes(T(0, 4, dtype=f32)) == b""            # (reshaped and cast first: still empty)
        assert binary.encode_to_bytes(T(0, dtype=i32)) == b""
        with pytest.raises(ValueError, match="an empty input is an empty FILE"):
            impl(ops.encode_stream)(T(0, dtype=i64), _handle())
    assert huff.decode_bytes(b"") is None and binary.decode_bytes(b"") is None


# ---- per-image routing for the length of one encode: the router config is the caller's again afterwards, whatever encode does
class _Stop(Exception):
    pass


class _Model:
    def __init__(self, params):
        ident = torch.nn.Identity
        self.encoder = type("Encoder", (), {})()
        if params is not None:
            self.encoder.router_config = {"params": params}
        self.encoder.conv_out_coarse, self.encoder.conv_out, self.encoder.conv_out_fine = ident(), ident(), ident()
        self.quantize = type("Quantizer", (), {})()
        self.quantize.embedding = type("Embedding", (), {"weight": torch.zeros(16, 4)})()
        self.quantize.embedding_counter = {str(i): torch.tensor([float(1 + i)]) for i in range(16)}
        self.seen = []

    def encode(self, x):
        rc = getattr(self.encoder, "router_config", None)
        self.seen.append(None if rc is None else rc["params"].get("per_image", "absent"))
        raise _Stop


@pytest.mark.parametrize("before", [{}, {"per_image": False}, {"per_image": True}])
def test_per_image_routing_is_forced_for_one_encode_and_restored(before):
    for run in (lambda m: cg.compress_batch(m, torch.zeros(1, 3, 16, 16)), lambda m: rate._encode_captured(m, torch.zeros(1, 3, 16, 16))):
        params = dict(before, coarse_grain_ratio=0.1)
        m = _Model(params)
        with pytest.raises(_Stop):
            run(m)
        assert m.seen == [True]
        assert params == dict(before, coarse_grain_ratio=0.1)
        heads = (m.encoder.conv_out_coarse, m.encoder.conv_out, m.encoder.conv_out_fine)
        assert all(len(mod._forward_hooks) == 0 for mod in heads)


def test_a_model_without_a_router_config():
    """compress_batch encodes it as it is; the rate search needs the config and says so with the attribute's name"""
    m = _Model(None)
    with pytest.raises(_Stop):
        cg.compress_batch(m, torch.zeros(1, 3, 16, 16))
    assert m.seen == [None]
    with pytest.raises(AttributeError, match="router_config"):
        rate._encode_captured(m, torch.zeros(1, 3, 16, 16))


# ---- the schema of every torch.ops.cgic op, as recorded before the bindings were merged
SCHEMAS = {
    "avg_pool": "cgic::avg_pool(Tensor x, SymInt k) -> Tensor",
    "compress_streams": "cgic::compress_streams(Tensor ind, Tensor mask_c, Tensor mask_m, Tensor mask_f, SymInt mode, SymInt table, Tensor(a6!)? hist) -> (Tensor, Tensor)",
    "container_pack": "cgic::container_pack(Tensor data, Tensor nbytes, SymInt mode, SymInt height, SymInt width, SymInt first_image_id) -> (Tensor, Tensor)",
    "decode_stream": "cgic::decode_stream(Tensor stream, SymInt nbytes, SymInt table) -> (Tensor, Tensor)",
    "decoder_blend_fine": "cgic::decoder_blend_fine(Tensor h, Tensor h_fine, Tensor mask_c, Tensor mask_m, Tensor mask_f) -> Tensor",
    "decoder_blend_medium": "cgic::decoder_blend_medium(Tensor h, Tensor h_medium, Tensor mask_c, Tensor mask_m) -> Tensor",
    "decompress_streams": "cgic::decompress_streams(Tensor data, Tensor nbytes, SymInt h, SymInt w, SymInt mode, SymInt table, Tensor codebook, str decoder) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "encode_stream": "cgic::encode_stream(Tensor symbols, SymInt table) -> (Tensor, Tensor)",
    "entropy_maps": "cgic::entropy_maps(Tensor x) -> (Tensor, Tensor)",
    "entropy_maps_reference_order": "cgic::entropy_maps_reference_order(Tensor x) -> (Tensor, Tensor)",
    "entropy_maps_u8": "cgic::entropy_maps_u8(Tensor frames) -> (Tensor, Tensor, Tensor)",
    "gather_grain_indices": "cgic::gather_grain_indices(Tensor ind_c, Tensor ind_m, Tensor ind_f, Tensor mask_c, Tensor mask_m, Tensor mask_f) -> Tensor",
    "grain_merge": "cgic::grain_merge(Tensor h_coarse, Tensor h_medium, Tensor h_fine, Tensor mask_c, Tensor mask_m, Tensor mask_f) -> Tensor",
    "index_histogram": "cgic::index_histogram(Tensor indices, Tensor(a1!) hist) -> ()",
    "partition_map": "cgic::partition_map(Tensor x, Tensor mask_c, Tensor mask_m, Tensor mask_f, bool frames) -> Tensor",
    "paste_tiles": "cgic::paste_tiles(Tensor[] pixels, SymInt H, SymInt W, SymInt N, SymInt tile, bool weighted, bool frames) -> Tensor",
    "rate_curve": "cgic::rate_curve(Tensor ind_c, Tensor ind_m, Tensor ind_f, Tensor e16, Tensor e8, float coarse, SymInt table) -> Tensor",
    "rate_table": "cgic::rate_table(Tensor ind_c, Tensor ind_m, Tensor ind_f, Tensor e16, Tensor e8, float[] coarse, float[] medium, bool per_image, SymInt table, Tensor? pixels=None) -> Tensor",
    "route_to_bpp": "cgic::route_to_bpp(Tensor ind_c, Tensor ind_m, Tensor ind_f, Tensor e16, Tensor e8, float coarse, Tensor budget, SymInt table) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "router": "cgic::router(Tensor e16, Tensor e8, float coarse_ratio, float medium_ratio, bool per_image, Tensor? pixels=None) -> (Tensor, Tensor, Tensor)",
    "vq_backward": "cgic::vq_backward(Tensor z, Tensor codebook, Tensor indices, Tensor g_zq, Tensor g_loss, float beta, bool legacy) -> (Tensor, Tensor)",
    "vq_forward": "cgic::vq_forward(Tensor z, Tensor codebook, float beta, bool legacy) -> (Tensor, Tensor, Tensor)",
    "vq_forward_route": "cgic::vq_forward_route(Tensor z, Tensor codebook, float beta, bool legacy, Tensor e16, Tensor e8, float coarse_ratio, float medium_ratio, bool per_image, Tensor? pixels=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
}


def test_op_schemas():
    got = {name: str(getattr(torch.ops.cgic, name).default._schema) for name in SCHEMAS}
    assert got == SCHEMAS
    defined = {n for n in dir(ops) if hasattr(getattr(ops, n), "_init_fn")}
    assert defined == set(SCHEMAS), "an op of ops.py has no recorded schema (or a recorded one is gone)"
