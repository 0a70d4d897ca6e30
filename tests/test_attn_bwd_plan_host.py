"""The launch plan of cgic_attention_backward (csrc/cgic_attn_bwd_plan.h) without a GPU: every check of the call and the geometry of
its three launches.  The header is plain C++17: tests/host/attn_bwd_plan_main.cpp is compiled with the host compiler alone -- once
plainly, once with -fsanitize=address,undefined -- and run as a program over the table below, whose rows were worked out by hand:
  pre   256 tokens per workgroup: grid ceil(N / 256) * B, no LDS; runs when dq or dk is wanted;
  dq    256 threads own 32 queries and walk the keys in tiles of 128: tiles = ceil(N / 32), grid = tiles * B;
  dkdv  256 threads own 32 keys and walk the queries in tiles of 128: tiles = ceil(N / 32), grid = tiles * B, run when dk or dv is wanted;
  LDS of dq and of dkdv alike = 32 * (2 * (C + pad) + (128 + pad)) elements of the operand type, pad = 8 (halves) or 1 (fp32):
      halves C=512: 32 * (1040 + 136) * 2 = 75264       halves C=256: 32 * (528 + 136) * 2 = 42496
      fp32   C=512: 32 * (1026 + 129) * 4 = 147840      fp32   C=256: 32 * (514 + 129) * 4 = 82304       (a compute unit has 163840)
  workspace = B * N * 4 bytes (delta) rounded up to 16;
  dq_vec (16-byte loads of k): halves only, N % 8 == 0, k 16-byte aligned, k's batch stride a multiple of 8 elements;
  dkdv_vec (of go and q): the same of both go and q."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, CAPACITY = 0, -1, -2, -5
F32, F16, BF16 = 0, 1, 2
ORDER = ("go", "q", "k", "v", "out", "lse", "dq", "dk", "dv", "ws")
BASE = {k: (i + 1) << 36 for i, k in enumerate(ORDER)}          # 64 GiB apart
LDS = {(F32, 256): 82304, (F32, 512): 147840, (F16, 256): 42496, (F16, 512): 75264, (BF16, 256): 42496, (BF16, 512): 75264}
SCALE = {256: 62500, 512: 44194}                                # C ** -0.5 in millionths


def case(name, want, dt_in, dt_grad, B, C, N, strides=None, scale=None, ws_bytes=-1, **addr):
    """addr: q=+8 style byte offsets from the tensor's base, or absolute addresses as ("abs", value); strides: elements (go, q, k, v),
    C * N when not given; ws_bytes -1: what the plan asks for"""
    a = dict(BASE)
    for key, v in addr.items():
        a[key] = v[1] if isinstance(v, tuple) else BASE[key] + v
    line = " ".join(str(v) for v in (dt_in, dt_grad, B, C, N, *(strides or (C * N,) * 4), SCALE.get(C, 100000) if scale is None else scale,
                                     *(a[key] for key in ORDER), ws_bytes))
    return pytest.param(line, want, id=name)


def plan(dt, B, C, N, vec=(0, 0), need=(1, 1, 1), **kw):
    dq, dk, dv = need
    t32 = -(-N // 32)
    return dict(form=1, pre_run=int(bool(dq or dk)), pre_threads=256, pre_grid=-(-N // 256) * B, dq_run=dq, dq_threads=256, dq_tiles=t32,
                dq_grid=t32 * B, dq_lds=LDS[dt, C], dkdv_run=int(bool(dk or dv)), dkdv_threads=256, dkdv_tiles=t32, dkdv_grid=t32 * B,
                dkdv_lds=LDS[dt, C], dq_vec=vec[0], dkdv_vec=vec[1], workspace=-(-B * N * 4 // 16) * 16, **kw)


def err(code, why):
    return dict(err=code, why=why)


PAIRS = ((F32, F32), (F16, F32), (F16, F16), (BF16, F32), (BF16, BF16))
NULL = ("abs", 0)
CASES = []
# ---- both widths, dense, N = 1 / 37 / 4096, each type pair
for dt_in, dt_grad in PAIRS:
    for C in (256, 512):
        for N in (1, 37, 4096):
            v = int(dt_in != F32 and N == 4096)
            CASES.append(case(f"dense-{dt_in}{dt_grad}-C{C}-N{N}", plan(dt_in, 3, C, N, (v, v)), dt_in, dt_grad, 3, C, N))
CASES += [
    case("spelled-out-bf16-512-4096-B2", dict(form=1, pre_run=1, pre_grid=32, dq_run=1, dq_tiles=128, dq_grid=256, dq_lds=75264, dkdv_run=1, dkdv_tiles=128,
                                              dkdv_grid=256, dkdv_lds=75264, dq_vec=1, dkdv_vec=1,
                                              workspace=32768), BF16, BF16, 2, 512, 4096),
    case("spelled-out-f32-512-37", dict(form=1, pre_grid=1, dq_tiles=2, dq_grid=2, dq_lds=147840, dkdv_tiles=2, dkdv_grid=2, dkdv_lds=147840,
                                        dq_vec=0, dkdv_vec=0, workspace=160), F32, F32, 1, 512, 37),
    case("spelled-out-f32-256-1-B3", dict(form=1, pre_grid=3, dq_grid=3, dkdv_grid=3, dq_lds=82304, workspace=16), F32, F32, 3, 256, 1),
    case("tile-768x768-N36864-bf16", plan(BF16, 1, 512, 36864, (1, 1)), BF16, BF16, 1, 512, 36864),
    case("tile-768x768-N36864-f32", dict(form=1, pre_grid=144, dq_grid=1152, dkdv_grid=1152, dq_lds=147840, dkdv_lds=147840, workspace=147456),
         F32, F32, 1, 512, 36864),
    case("tile-592x768-N1776", plan(F16, 1, 512, 1776, (1, 1)), F16, F16, 1, 512, 1776),
    case("empty-batch", dict(form=0, pre_grid=0, dq_grid=0, dkdv_grid=0, workspace=0), F32, F32, 0, 256, 37, **{k: NULL for k in ORDER}),
    case("scale-0", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, scale=0),
    # ---- which outputs are wanted
    case("no-output-is-a-no-op", dict(form=0), F32, F32, 2, 256, 37, dq=NULL, dk=NULL, dv=NULL),
    case("no-output-looks-at-nothing-else", dict(form=0), F32, F32, 2, 256, 37, **{k: NULL for k in ORDER}),
    case("only-dq", plan(F32, 2, 256, 37, need=(1, 0, 0)), F32, F32, 2, 256, 37, dk=NULL, dv=NULL),
    case("only-dk", plan(F32, 2, 256, 37, need=(0, 1, 0)), F32, F32, 2, 256, 37, dq=NULL, dv=NULL),
    case("only-dv-needs-no-delta", plan(F32, 2, 256, 37, need=(0, 0, 1)), F32, F32, 2, 256, 37, dq=NULL, dk=NULL),
    case("dk-and-dv", plan(F32, 2, 256, 37, need=(0, 1, 1)), F32, F32, 2, 256, 37, dq=NULL),
    case("dq-and-dv", plan(F32, 2, 256, 37, need=(1, 0, 1)), F32, F32, 2, 256, 37, dk=NULL),
    # ---- strided batch: the thirds of one [B, 3C, N] tensor (q at the base, k and v C*N and 2*C*N elements behind it), go dense
    case("qkv-views-f16-4096", plan(F16, 3, 512, 4096, (1, 1)), F16, F16, 3, 512, 4096, strides=(512 * 4096,) + (3 * 512 * 4096,) * 3,
         k=("abs", BASE["q"] + 512 * 4096 * 2), v=("abs", BASE["q"] + 2 * 512 * 4096 * 2)),
    case("qkv-views-f32-37", plan(F32, 3, 256, 37), F32, F32, 3, 256, 37, strides=(256 * 37,) + (3 * 256 * 37,) * 3,
         k=("abs", BASE["q"] + 256 * 37 * 4), v=("abs", BASE["q"] + 2 * 256 * 37 * 4)),
    # ---- the 16-byte loads
    case("vec-N-8", plan(F16, 1, 256, 8, (1, 1)), F16, F16, 1, 256, 8),
    case("narrow-N-12", plan(F16, 1, 256, 12, (0, 0)), F16, F16, 1, 256, 12),
    case("narrow-odd-N-111", plan(BF16, 1, 256, 111, (0, 0)), BF16, BF16, 1, 256, 111),
    case("k+2-narrows-dq", plan(F16, 1, 256, 256, (0, 1)), F16, F16, 1, 256, 256, k=2),
    case("k+16-does-not", plan(F16, 1, 256, 256, (1, 1)), F16, F16, 1, 256, 256, k=16),
    case("q+2-narrows-dkdv", plan(F16, 1, 256, 256, (1, 0)), F16, F16, 1, 256, 256, q=2),
    case("go+8-narrows-dkdv", plan(F16, 1, 256, 256, (1, 0)), F16, F16, 1, 256, 256, go=8),
    case("v+2-narrows-nothing", plan(F16, 1, 256, 256, (1, 1)), F16, F16, 1, 256, 256, v=2),
    case("k-stride+4-narrows-dq", plan(F16, 2, 256, 256, (0, 1)), F16, F16, 2, 256, 256, strides=(65536, 65536, 65540, 65536)),
    case("go-stride+4-narrows-dkdv", plan(F16, 2, 256, 256, (1, 0)), F16, F16, 2, 256, 256, strides=(65540, 65536, 65536, 65536)),
    case("strides+8-keep-both", plan(F16, 2, 256, 256, (1, 1)), F16, F16, 2, 256, 256, strides=(65544,) * 4),
    case("f32-never", plan(F32, 1, 256, 256, (0, 0)), F32, F32, 1, 256, 256),
]
# ---- the refusals, in the order of the checks
PAIR = "attention_backward: grad_dtype %d with in_dtype %d (CGIC_DT_F32 or the inputs' own type)"
WIDTH = "attention_backward: %d channels (built for 256 and 512, the model's widths)"
ALIGN = "attention_backward: a pointer is not aligned to its %d-byte element"
WS = "attention_backward: workspace of %d bytes, need 304 (cgic_attention_backward_workspace_bytes)"        # [2, 37] floats: 296 -> 304
CASES += [
    case("types-30", err(INVALID, "attention_backward: in_dtype 3 (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)"), 3, F32, 1, 256, 37),
    case("types-01-f32-in-half-grads", err(UNSUPPORTED, PAIR % (1, 0)), F32, F16, 1, 256, 37),
    case("types-02", err(UNSUPPORTED, PAIR % (2, 0)), F32, BF16, 1, 256, 37),
    case("types-12", err(UNSUPPORTED, PAIR % (2, 1)), F16, BF16, 1, 256, 37),
    case("types-1-1", err(INVALID, PAIR % (-1, 1)), F16, -1, 1, 256, 37),
    case("shape-B-1", err(INVALID, "attention_backward: q, k, v [-1,256,37]"), F32, F32, -1, 256, 37),
    case("shape-N0", err(INVALID, "attention_backward: q, k, v [1,256,0]"), F32, F32, 1, 256, 0),
    case("shape-C0", err(INVALID, "attention_backward: q, k, v [1,0,37]"), F32, F32, 1, 0, 37),
    case("width-48", err(UNSUPPORTED, WIDTH % 48), F32, F32, 1, 48, 37),
    case("width-128", err(UNSUPPORTED, WIDTH % 128), F16, F16, 1, 128, 37),
    case("width-1024", err(UNSUPPORTED, WIDTH % 1024), BF16, BF16, 1, 1024, 37),
    case("grid-2^31", err(UNSUPPORTED, "attention_backward: 1048576 images of 65536 tokens are beyond a grid of 2^31 workgroups"), F16, F16, 1 << 20, 256, 65536),
    case("scale-negative", err(INVALID, "attention_backward: scale -0.0625 (finite, not negative)"), F32, F32, 1, 256, 37, scale=-62500),
    case("stride-go-short", err(INVALID, "attention_backward: batch strides 9471, 9472, 9472, 9472 below C * N = 9472 elements"), F32, F32, 2, 256, 37,
         strides=(9471, 9472, 9472, 9472)),
    case("stride-v-short", err(INVALID, "attention_backward: batch strides 9472, 9472, 9472, 0 below C * N = 9472 elements"), F32, F32, 2, 256, 37,
         strides=(9472, 9472, 9472, 0)),
    case("stride-exact", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, strides=(9472,) * 4),
    # ---- a stride that would wrap the extents of the aliasing check: 2^59 / B elements is the cap
    # (at the cap the extent of k is 2^60 bytes, computed without wrapping: it covers every tensor behind k)
    case("stride-k-at-the-cap", err(INVALID, "attention_backward: dq overlaps k"), F32, F32, 2, 256, 37, strides=(9472, 9472, 1 << 58, 9472)),
    case("stride-k-beyond-the-cap", err(INVALID, "attention_backward: batch strides 9472, 9472, 288230376151711745, 9472 beyond 2^59 / B = 288230376151711744 elements"),
         F32, F32, 2, 256, 37, strides=(9472, 9472, (1 << 58) + 1, 9472)),
    case("stride-go-2^62", err(INVALID, "attention_backward: batch strides 4611686018427387904, 9472, 9472, 9472 beyond 2^59 / B = 192153584101141162 elements"),
         F32, F32, 3, 256, 37, strides=(1 << 62, 9472, 9472, 9472)),
    case("stride-2^62-of-one-image-is-never-used", err(INVALID, "attention_backward: batch strides 9472, 9472, 9472, 4611686018427387904 beyond 2^59 / B = 576460752303423488 elements"),
         F32, F32, 1, 256, 37, strides=(9472, 9472, 9472, 1 << 62)),
]
for name in ("go", "q", "k", "v", "out", "lse"):
    CASES.append(case(f"NULL-{name}", err(INVALID, "attention_backward: NULL input"), F32, F32, 1, 256, 37, **{name: NULL}))
CASES += [
    case("misaligned-q16+1", err(INVALID, ALIGN % 2), F16, F32, 1, 256, 37, q=1),
    case("misaligned-go32+2", err(INVALID, ALIGN % 4), F32, F32, 1, 256, 37, go=2),
    case("misaligned-out16+1", err(INVALID, ALIGN % 2), BF16, BF16, 1, 256, 37, out=1),
    case("misaligned-lse+2", err(INVALID, ALIGN % 4), F16, F16, 1, 256, 37, lse=2),
    case("misaligned-dk32+2-of-half-inputs", err(INVALID, ALIGN % 4), BF16, F32, 1, 256, 37, dk=2),
    case("aligned-dk16+2", plan(BF16, 1, 256, 37), BF16, BF16, 1, 256, 37, dk=2),
    # ---- the workspace: [2, 37] floats
    case("ws-NULL", err(CAPACITY, WS % 0), F32, F32, 2, 256, 37, ws=NULL),
    case("ws-short", err(CAPACITY, WS % 303), F32, F32, 2, 256, 37, ws_bytes=303),
    case("ws-exact", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, ws_bytes=304),
    case("ws-larger", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, ws_bytes=4096),
    case("ws+8", err(INVALID, "attention_backward: workspace is not 16-byte aligned"), F32, F32, 2, 256, 37, ws=8),
    case("ws+16", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, ws=16),
]
# ---- aliasing: [2,256,37] fp32 is 75776 bytes, its lse 296, its workspace 304: each output on each input and on the workspace
for o in ("dq", "dk", "dv"):
    for i in ("go", "q", "k", "v", "out", "lse", "ws"):
        CASES.append(case(f"{o}-is-{i}", err(INVALID, f"attention_backward: {o} overlaps {'the workspace' if i == 'ws' else i}"), F32, F32, 2, 256, 37,
                          **{o: ("abs", BASE[i])}))
CASES += [
    case("dq-ends-in-v", err(INVALID, "attention_backward: dq overlaps v"), F32, F32, 2, 256, 37, dq=("abs", BASE["v"] - 75776 + 4)),
    case("dq-before-v", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, dq=("abs", BASE["v"] - 75776)),
    case("dq-behind-k", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, dq=("abs", BASE["k"] + 75776)),
    case("dq-in-the-gap-of-strided-k", err(INVALID, "attention_backward: dq overlaps k"), F32, F32, 2, 256, 37, strides=(9472, 9472, 1 << 20, 9472),
         dq=("abs", BASE["k"] + 75776)),
    case("dv-in-the-gap-of-strided-go", err(INVALID, "attention_backward: dv overlaps go"), F32, F32, 2, 256, 37, strides=(1 << 20, 9472, 9472, 9472),
         dv=("abs", BASE["go"] + 75776)),
    case("dk-ends-in-lse", err(INVALID, "attention_backward: dk overlaps lse"), F32, F32, 2, 256, 37, dk=("abs", BASE["lse"] + 292)),
    case("dk-behind-lse", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, dk=("abs", BASE["lse"] + 296)),
    case("dv-in-the-workspace's-last-byte", err(INVALID, "attention_backward: dv overlaps the workspace"), F32, F32, 2, 256, 37, dv=("abs", BASE["ws"] + 300)),
    case("dv-behind-the-needed-workspace", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, dv=("abs", BASE["ws"] + 304), ws_bytes=4096),
    case("dk-is-dq", err(INVALID, "attention_backward: dk overlaps dq"), F32, F32, 2, 256, 37, dk=("abs", BASE["dq"])),
    case("dv-is-dq", err(INVALID, "attention_backward: dv overlaps dq"), F32, F32, 2, 256, 37, dv=("abs", BASE["dq"] + 75772)),
    case("dv-is-dk", err(INVALID, "attention_backward: dv overlaps dk"), F32, F32, 2, 256, 37, dv=("abs", BASE["dk"])),
    case("dv-behind-dk", plan(F32, 2, 256, 37), F32, F32, 2, 256, 37, dv=("abs", BASE["dk"] + 75776)),
    case("an-unwanted-output-overlaps-nothing", plan(F32, 2, 256, 37, need=(1, 0, 1)), F32, F32, 2, 256, 37, dk=NULL, dv=("abs", BASE["dk"])),
]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "attn_bwd_plan_main.cpp"), "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], input="\n".join(c.values[0] for c in CASES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    parsed = {}
    for c, line in zip(CASES, lines):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            parsed[c.id] = {k: int(v) for k, v in (t.split("=", 1) for t in line.split())}
    return parsed


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("attn_bwd_plan"), [], "attn_bwd_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_attn_bwd_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_no_built_shape_exceeds_the_lds_of_a_compute_unit(plans):
    """the plan refuses beyond 160 KiB; both kernels of every built width and type stay under it, the fp32 one at C = 512 by 16000 bytes
    -- a second tile (P and dS side by side) would not have fitted"""
    for key, lds in LDS.items():
        assert lds <= 160 * 1024
    assert LDS[F32, 512] + 32 * 129 * 4 > 160 * 1024


def test_attn_bwd_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "attn_bwd_plan_main_san")
    assert _run(exe) == plans


def test_the_library_answers_as_the_plan_does():
    """cgic_attention_backward_supported / _workspace_bytes are the plan's shape part, and a refused call enqueues nothing: it can be
    made without a device, with made-up addresses (never dereferenced)"""
    import control_gic_amd as cg
    from control_gic_amd import _lib
    lib = _lib.lib()
    assert lib.cgic_abi_version() >= 20
    for dt_in, dt_grad in PAIRS:
        for C in (256, 512):
            assert lib.cgic_attention_backward_supported(dt_in, dt_grad, 3, C, 37) == 1
    assert lib.cgic_attention_backward_supported(F32, F32, 1, 48, 37) == 0 and lib.cgic_attention_backward_supported(F32, F16, 1, 256, 37) == 0
    assert lib.cgic_attention_backward_supported(F16, F16, 1 << 20, 256, 65536) == 0
    assert lib.cgic_attention_backward_supported(3, F32, 1, 256, 37) == INVALID
    assert "in_dtype 3" in lib.cgic_last_error().decode()
    assert lib.cgic_attention_backward_supported(F32, F32, 1, 256, 0) == INVALID
    size = lib.cgic_attention_backward_workspace_bytes
    assert size(BF16, 2, 512, 4096) == 32768 and size(F32, 2, 256, 37) == 304 and size(F32, 1, 48, 37) == 0 and size(F16, 0, 256, 37) == 0
    assert size(F32, 1, 512, 36864) == 147456 <= 64 * 36864 + 4096                  # within 64 bytes per token and image plus 4 KiB

    def refused(code, text, *args):
        with pytest.raises(cg.CgicError) as got:
            _lib.call("cgic_attention_backward", *args)
        assert got.value.code == code and text in str(got.value), str(got.value)

    go, q, k, v, out, lse, dq, dk, dv, ws = (BASE[n] for n in ORDER)
    n = 256 * 37

    def args(**kw):
        a = dict(go=go, q=q, k=k, v=v, out=out, lse=lse, dt=F32, B=1, C=256, N=37, sg=n, sq=n, sk=n, sv=n, scale=0.0625, dq=dq, dk=dk, dv=dv, gdt=F32,
                 ws=ws, ws_bytes=160)
        a.update(kw)
        return (a["go"], a["q"], a["k"], a["v"], a["out"], a["lse"], a["dt"], a["B"], a["C"], a["N"], a["sg"], a["sq"], a["sk"], a["sv"], a["scale"],
                a["dq"], a["dk"], a["dv"], a["gdt"], a["ws"], a["ws_bytes"], None)

    refused(UNSUPPORTED, WIDTH % 48, *args(C=48))
    refused(UNSUPPORTED, PAIR % (1, 0), *args(gdt=F16))
    refused(INVALID, "attention_backward: dq overlaps k", *args(dq=k))
    refused(INVALID, "attention_backward: dv overlaps the workspace", *args(dv=ws))
    refused(INVALID, "attention_backward: NULL input", *args(lse=None))
    refused(INVALID, "below C * N", *args(B=2, sk=n - 1))
    refused(INVALID, "not aligned to its 2-byte element", *args(dt=F16, gdt=F16, q=q + 1))
    refused(INVALID, "scale nan", *args(scale=float("nan")))
    refused(CAPACITY, "workspace of 100 bytes, need 160", *args(ws_bytes=100))
    assert _lib.call("cgic_attention_backward", *args(B=0, go=None, q=None, k=None, v=None, out=None, lse=None, dq=None, dk=None, dv=None, ws=None, ws_bytes=0)) == OK
    assert _lib.call("cgic_attention_backward", *args(dq=None, dk=None, dv=None)) == OK                    # no output wanted: a no-op
