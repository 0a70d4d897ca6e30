"""The launch plan of cgic_decompress_streams (csrc/cgic_decode_plan.h) without a GPU: which decoder path and merge form a shape
takes, the grids and the LDS sizes.  The header is plain C++17: tests/host/decode_plan_main.cpp is compiled with the host compiler
alone and run over the table below, whose rows were worked out by hand from the arithmetic of the host path."""
import os
import shutil
import subprocess

import pytest

import long_codes_ref as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, LATENCY, THROUGHPUT = 0, 1, 2
ERR_UNSUPPORTED, ERR_CAPACITY = -2, -5
LDS_DECODER = 90000            # stands for decoder_lds_bytes(true); the plan only passes it on (lds_d) and takes the maximum (lds_f)

# 256 CUs, share 1.0, K = 1024, z_q given, max_len 20, lut_bits 13 unless a row says otherwise; h x w are latent grids
DEFAULTS = dict(slot=1 << 20, K=1024, has_zq=1, max_len=20, lut_bits=13, cus=256, share=1.0, no_fuse=0, lds_decoder=LDS_DECODER)


def _case(name, B, h, w, mode, want, **shape):
    return pytest.param(dict(DEFAULTS, B=B, h=h, w=w, mode=mode, **shape), want, id=name)


def _merge(nbands, active, stage_cb, stage_sym, band_syms, lds_m):
    return dict(nbands=nbands, active=active, stage_cb=stage_cb, stage_sym=stage_sym, band_syms=band_syms, lds_m=lds_m)


def _fused(grid, ndec, *merge):
    return dict(decoder="fused", grid=grid, ndec=ndec, **_merge(*merge))


def _split(ndec, form, *merge):
    return dict(decoder="split", merge=form, ndec=ndec, split_batch=1365, **_merge(*merge))


def _image(threads, stage_cap, chunk_cap, lds_ss, form, *merge):
    return dict(decoder="image", merge=form, ndec=1, image_threads=threads, stage_cap=stage_cap, chunk_cap=chunk_cap, lds_ss=lds_ss,
                **_merge(*merge))


CASES = [
    _case("64x64x64-auto", 64, 64, 64, AUTO, _split(4, "bands", 4, 4, 1, 1, 0, 27632)),
    _case("64x64x64-latency", 64, 64, 64, LATENCY, _split(4, "bands", 4, 4, 1, 1, 0, 27632)),
    _case("64x64x64-throughput", 64, 64, 64, THROUGHPUT, _image(256, 13616, 1696, 51472, "one_band", 4, 4, 1, 1, 0, 27632)),
    _case("1x64x64-auto", 1, 64, 64, AUTO, _fused(20, 4, 16, 16, 1, 1, 0, 27632)),
    _case("1x64x64-latency", 1, 64, 64, LATENCY, _fused(20, 4, 16, 16, 1, 1, 0, 27632)),
    _case("8x64x64-auto", 8, 64, 64, AUTO, _fused(96, 4, 8, 8, 1, 1, 0, 27632)),
    _case("8x64x64-latency", 8, 64, 64, LATENCY, _fused(160, 4, 16, 16, 1, 1, 0, 27632)),
    _case("16x64x64-auto", 16, 64, 64, AUTO, _fused(128, 4, 4, 4, 1, 1, 0, 27632)),
    _case("16x64x64-latency", 16, 64, 64, LATENCY, _fused(192, 4, 8, 8, 1, 1, 0, 27632)),
    _case("1x192x192-auto", 1, 192, 192, AUTO, _fused(48, 16, 32, 24, 1, 0, 2024, 24768)),
    _case("1x192x192-latency", 1, 192, 192, LATENCY, _fused(48, 16, 32, 24, 1, 0, 2024, 24768)),
    _case("1x192x192-throughput", 1, 192, 192, THROUGHPUT, _split(24, "bands", 32, 24, 1, 0, 2024, 24768)),
    _case("4x192x192-auto", 4, 192, 192, AUTO, _fused(128, 16, 16, 16, 1, 0, 3032, 26784)),
    _case("4x192x192-latency", 4, 192, 192, LATENCY, _fused(192, 16, 32, 24, 1, 0, 2024, 24768)),
    _case("6x128x192-auto", 6, 128, 192, AUTO, _fused(120, 16, 4, 4, 1, 0, 8072, 35424)),
    _case("6x128x192-latency", 6, 128, 192, LATENCY, _fused(192, 16, 16, 16, 1, 0, 2024, 23328)),
    _case("6x128x192-throughput", 6, 128, 192, THROUGHPUT, _image(1024, 80816, 10096, 143872, "bands", 32, 32, 1, 0, 1016, 21312)),
    _case("1x340x512-auto", 1, 340, 512, AUTO, _fused(80, 16, 64, 43, 1, 0, 5384, 47568)),
    # the self-synchronising decoder's LDS does not fit: the split-stream decoder
    _case("1x340x512-throughput", 1, 340, 512, THROUGHPUT, _split(24, "bands", 64, 43, 1, 0, 5384, 47568)),
    _case("1x4x4-auto", 1, 4, 4, AUTO, _fused(8, 4, 4, 1, 1, 0, 29, 16482)),
    _case("1x8x4-throughput", 1, 8, 4, THROUGHPUT, _image(256, 288, 32, 33152, "one_band", 4, 2, 1, 1, 0, 16508)),
    _case("2x12x20-auto", 2, 12, 20, AUTO, _fused(16, 4, 4, 3, 1, 0, 113, 16662)),
    # beyond one ticket request: never fused, the split path in launches of 1365 images (1365 + 35)
    _case("1400x16x16-auto", 1400, 16, 16, AUTO, _split(4, "bands", 4, 4, 1, 1, 0, 17108)),
    _case("1x64x64-max_len70", 1, 64, 64, AUTO, dict(decoder="serial", merge="bands", ndec=3, **_merge(16, 16, 1, 1, 0, 27632)), max_len=70),
    _case("2x64x64-share0.25", 2, 64, 64, AUTO, _fused(24, 4, 8, 8, 1, 1, 0, 27632), share=0.25),
    # the dev knob: nothing fuses, the bands are doubled as far as the rows allow
    _case("1x64x64-latency-knob", 1, 64, 64, LATENCY, _split(4, "bands", 16, 16, 1, 1, 0, 27632), no_fuse=1),
    # no z_q: no codebook in LDS (496 bytes of bitsets + 5376 symbols of 2 bytes)
    _case("1x64x64-no_zq", 1, 64, 64, AUTO, _fused(20, 4, 16, 16, 0, 1, 0, 11248), has_zq=0),
    # a decoder that needs less LDS than the merge: the fused launch takes the merge's
    _case("1x64x64-small-decoder", 1, 64, 64, AUTO, dict(_fused(20, 4, 16, 16, 1, 1, 0, 27632), lds_f=27632), lds_decoder=1000),
    # 3 x (2813 + 11250) words of bitsets + 4 = 168772 bytes > 150 KB
    _case("1x1200x1200-bitsets", 1, 1200, 1200, AUTO, dict(err=ERR_UNSUPPORTED, why="grid too large for the mask bitsets")),
    # a 64x64 grid's medium mask stream is staged as 32 + 2 words = 136 bytes
    _case("1x64x64-slot128", 1, 64, 64, AUTO, dict(err=ERR_CAPACITY, why="slot smaller than a mask stream"), slot=128),
    _case("1x64x64-slot144", 1, 64, 64, AUTO, _fused(20, 4, 16, 16, 1, 1, 0, 27632), slot=144),
]


# ---- code tables of 14 to 65 bits: every (B, h, w, longest code, decoder argument) that tests/test_long_codes.py runs, with the path
# it must take (long_codes_ref.CODEC_CASES and FORM_CASES, worked out by hand there), so that "this case reaches the image decoder" is
# a checked fact.  K follows the table; the slot is a 64-bit stream of the grid.
_LONG_PATHS = {"image256": dict(decoder="image", ndec=1, image_threads=256), "image1024": dict(decoder="image", ndec=1, image_threads=1024),
               "split4": dict(decoder="split", ndec=4, split_batch=1365), "split24": dict(decoder="split", ndec=24, split_batch=1365),
               "serial": dict(decoder="serial", ndec=3)}


def _long_code_rows():
    rows = [(lc.case_id(K, L, B, h, w), K, L, B, h, w, paths) for K, L, B, h, w, paths in lc.CODEC_CASES]
    rows += [(f"form-{form}-{lc.case_id(1024, 64, B, h, w)}", 1024, 64, B, h, w, paths) for form, B, h, w, paths in lc.FORM_CASES]
    for name, K, L, B, h, w, paths in rows:
        for mode, path in zip((AUTO, LATENCY, THROUGHPUT), paths):
            # the fused launch: 4 decoder workgroups per image up to 64x64, 16 beyond
            want = dict(decoder="fused", ndec=4 if h * w <= 64 * 64 else 16) if path == "fused" else _LONG_PATHS[path]
            yield _case(f"{name}-{lc.DECODERS[mode]}", B, h, w, mode, want, K=K, max_len=L, slot=8 * h * w + 16 + 1024)


CASES += list(_long_code_rows())
CASES += [
    # the plan's boundary between 64 bits and 65: the same shapes a bit apart
    _case("1x64x64-max_len64", 1, 64, 64, AUTO, _fused(20, 4, 16, 16, 1, 1, 0, 27632), max_len=64),
    _case("1x64x64-max_len65", 1, 64, 64, AUTO, dict(decoder="serial", merge="bands", ndec=3, **_merge(16, 16, 1, 1, 0, 27632)), max_len=65),
    # 64 bits x 5376 symbols + 192 = 344 256 bits: a stage of 43 032 + 144 bytes and three chunk tables of 5379 + 8, each rounded up
    # to 16, behind the 32 KB LUT
    _case("40x64x64-max_len64-throughput", 40, 64, 64, THROUGHPUT, _image(256, 43184, 5392, 92128, "one_band", 8, 8, 1, 1, 0, 27632), max_len=64),
    _case("40x64x64-max_len65-throughput", 40, 64, 64, THROUGHPUT, dict(decoder="serial", merge="one_band", ndec=3), max_len=65),
    # the self-synchronising decoder's LDS at 64 bits: 21 symbols per coarse cell.  522 cells (72x116): 701 760 bits, a stage of
    # 87 720 + 144 -> 87 872 bytes and chunk tables of 10 965 + 8 -> 10 976: 32 768 + 87 872 + 32 928 = 153 568 <= 153 600.
    # 523 cells (4x2092, a prime): 703 104 bits, 88 032 + 3 x 11 008 + 32 768 = 153 824: the split decoder, as for 72x120
    _case("1x72x116-max_len64-largest-image", 1, 72, 116, THROUGHPUT, dict(decoder="image", ndec=1, image_threads=1024, stage_cap=87872,
                                                                         chunk_cap=10976, lds_ss=153568), max_len=64),
    _case("1x4x2092-max_len64-next-cell", 1, 4, 2092, THROUGHPUT, dict(decoder="split", ndec=24, lds_ss=0), max_len=64),
    _case("1x72x120-max_len64-next-grid", 1, 72, 120, THROUGHPUT, dict(decoder="split", ndec=24, lds_ss=0), max_len=64),
]


# ---- malformed streams: every (B, h, w, table, decoder argument) that tests/test_malformed_streams.py runs, with the path it is meant
# to reach (malformed_ref.GPU_CASES), and the merge form where the case is there for it.  The slot is the library's for the table.
def _malformed_rows():
    import malformed_ref as mr
    for table, B, h, w, paths in mr.GPU_CASES:
        K, L = mr.table_shape(table)
        for mode, path in zip((AUTO, LATENCY, THROUGHPUT), paths):
            want = dict(decoder="fused", ndec=4 if h * w <= 64 * 64 else 16) if path == "fused" else dict(_LONG_PATHS[path])
            # the symbols of a grid up to 64x96 are staged in LDS whole, those of 192x192 band by band; "throughput" merges a grid up
            # to 64x64 in one band of 1024 threads
            want["stage_sym"] = int(h * w <= 64 * 132)
            if h * w == 192 * 192:
                assert path != "image256"
                want["band_syms"] = 2024
            if path != "fused":
                want["merge"] = "one_band" if mode == THROUGHPUT and h * w <= 64 * 64 else "bands"
            yield _case(f"malformed-{mr.gpu_case_id(table, B, h, w)}-{lc.DECODERS[mode]}", B, h, w, mode, want, K=K, max_len=L,
                        lut_bits=min(L, lc.LUT_BITS), slot=mr.slot_bytes(L, h, w))
            if mode == AUTO:                  # the same call without z_q (the index-outside-the-codebook case runs both ways)
                yield _case(f"malformed-{mr.gpu_case_id(table, B, h, w)}-auto-no_zq", B, h, w, mode, {k: v for k, v in want.items() if k != "band_syms"},
                            K=0, has_zq=0, max_len=L, lut_bits=min(L, lc.LUT_BITS), slot=mr.slot_bytes(L, h, w))


CASES += list(_malformed_rows())
FIELDS = ("B", "h", "w", "slot", "K", "has_zq", "max_len", "lut_bits", "mode", "cus", "share", "no_fuse", "lds_decoder")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every case of the table through ONE run of the compiled program: {case id: parsed output line}"""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp_path_factory.mktemp("decode_plan") / "decode_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", os.path.join(ROOT, "tests", "host", "decode_plan_main.cpp"), "-o", exe])
    text = "\n".join(" ".join(str(c.values[0][f]) for f in FIELDS) for c in CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    parsed = {}
    for c, line in zip(CASES, out):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            kv = dict(t.split("=", 1) for t in line.split())
            parsed[c.id] = {k: v if k in ("decoder", "merge") else int(v) for k, v in kv.items()}
    return parsed


@pytest.mark.parametrize("shape,want", CASES)
def test_decode_plan(plans, request, shape, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got["err"] == want["err"] and want["why"] in got["why"]
        return
    assert "err" not in got, got
    want = dict(want)
    grid = want.pop("grid", None)
    if grid is not None:                                  # the fused launch: decoder workgroups and bands of every image
        assert shape["B"] * (got["ndec"] + got["nbands"]) == grid
    assert {k: got[k] for k in want} == want
    assert got["lds_d"] == shape["lds_decoder"] and got["lds_f"] == max(got["lds_d"], got["lds_m"])
    if got["decoder"] != "image":
        assert got["lds_ss"] == got["stage_cap"] == got["chunk_cap"] == got["image_threads"] == 0
    if got["decoder"] != "split":
        assert got["split_batch"] == 0
