"""The launch plans of the encode host path (csrc/cgic_encode_plan.h) without a GPU: router_plan (ranks, index magic, LDS stage, row
bands, refinement queues) and vq_plan (filter path or exact loop, kernel variant, the VQ shares beside the router's workgroups,
LDS, tickets).  The header is plain C++17: tests/host/encode_plan_main.cpp is compiled with the host compiler alone and run over
the tables below, whose rows were worked out by hand from the arithmetic of the host path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
KID_AL, KID_UN = 5, 6          # stand for KID_VQF_ROUTER_AL / _UN: the plan only passes them on
LDS_FILTER = 54272             # vqf_lds_bytes(1024): 32 KB of fp16 operands + 16.5 KB of padded rows + 4.5 KB of norms
ROUTER_LDS = 35528             # a refined 16x16 segment: 4096 + 32 + 4 * 1280 + 16 + 26264
LDS_SHARED, LDS_REFINE = 4096, 26264      # kRouterSharedBytes, sizeof(RefineShared)

# ---- vq_plan: 256 CUs, share 1.0 and no group recorded, K = 1024, no conv, no knobs unless a row says otherwise -------------------
V_DEFAULTS = dict(K=1024, conv=0, loss=0, perm=0, cus=256, share=1.0, recording=0, R=0, router_lds=ROUTER_LDS, queues=0,
                  lds_filter=LDS_FILTER, kid_al=KID_AL, kid_un=KID_UN, exact=0, zt=0, wgs_per_cu=0, nosplit=0, ge=0)
V_FIELDS = ("N", "hw", "K", "conv", "loss", "perm", "cus", "share", "recording", "R", "router_lds", "queues", "lds_filter", "kid_al",
            "kid_un", "exact", "zt", "wgs_per_cu", "nosplit", "ge")


def _v(name, N, hw, want, **shape):
    return pytest.param("V", dict(V_DEFAULTS, N=N, hw=hw, **shape), want, id="vq-" + name)


def _filter(nblk, n_early, g_early, g_late, behind, grid, **more):
    want = dict(path="filter", nblk=nblk, n_early=n_early, g_early=g_early, g_late=g_late, grid=grid, threads=512, tickets=0, tail_mode=0)
    if behind is not None:
        want["behind"] = behind
    return dict(want, **more)


def _exact(zt, nblk, grid, lds, **more):
    return dict(dict(path="exact", zt=zt, nblk=nblk, grid=grid, lds=lds, threads=256, n_early=0, g_early=0, g_late=0, tickets=0,
                     tail_mode=0, kid=0), **more)


# a launch group's share counts while the group is recorded
def _share(x):
    return dict(share=x, recording=1)


V_CASES = [
    # ---- the filter path: N vectors, hw vectors per image, R router workgroups
    _v("64x64x64-fused-loss", 262144, 4096, _filter(256, 256, 16, 16, 1, 320, tickets=33, tail_mode=2, variant="router", kid=KID_AL,
                                                     lds=LDS_FILTER, aligned=1), R=64, loss=1),
    _v("64x64x64", 262144, 4096, _filter(256, 256, 16, 16, None, 256, variant="plain", kid=0, lds=LDS_FILTER)),
    _v("16x128x128", 262144, 16384, _filter(256, 192, 20, 4, 0, 320, variant="router", kid=KID_AL), R=64),
    _v("8x192x192", 294912, 36864, _filter(256, 192, 24, 0, 0, 320), R=64),
    _v("8x192x192-share0.5", 294912, 36864, _filter(128, 128, 36, 36, 1, 192), R=64, **_share(0.5)),
    _v("32x96x96", 294912, 9216, _filter(256, 256, 18, 18, 1, 320), R=64),
    _v("2x340x512", 348160, 174080, _filter(256, 240, 24, 0, 0, 272), R=16),
    _v("16x64x64-share0.25", 65536, 4096, _filter(64, 64, 16, 16, 1, 80), R=16, **_share(0.25)),
    _v("one-image", 4096, 4096, _filter(64, 64, 1, 1, 1, 65), R=1),
    _v("65-vectors-unaligned", 65, 65, _filter(2, 2, 1, 1, 1, 3, aligned=0, kid=KID_UN), R=1),
    _v("300-images", 1228800, 4096, _filter(256, 256, 75, 75, 1, 556), R=300),
    # ---- a permuted prepared image: the PERM kernels read K keys behind the codebook image
    _v("perm", 262144, 4096, _filter(256, 256, 16, 16, None, 256, variant="perm", lds=LDS_FILTER + 4096, kid=0), perm=1),
    _v("perm-router", 262144, 4096, _filter(256, 256, 16, 16, 1, 320, variant="router_perm", lds=LDS_FILTER + 4096, kid=0), perm=1, R=64),
    # ... but the plain kernels inside a launch group and with a fused quant_conv
    _v("perm-recording", 262144, 4096, _filter(256, 256, 16, 16, 1, 320, variant="router", lds=LDS_FILTER, kid=KID_AL), perm=1, R=64,
       **_share(1.0)),
    _v("perm-conv", 262144, 4096, _filter(256, 256, 16, 16, None, 256, variant="plain", lds=LDS_FILTER, kid=0), perm=1, conv=1),
    # a fused quant_conv has no recorded form
    _v("conv-router", 262144, 4096, _filter(256, 256, 16, 16, 1, 320, variant="router", kid=0), conv=1, R=64),
    # the router's refinement queues: the SPLIT instantiation
    _v("router-queues", 262144, 4096, _filter(256, 256, 16, 16, 1, 320, variant="router_split", kid=KID_AL), R=64, queues=1),
    # ---- dev knobs
    _v("16x128x128-nosplit", 262144, 16384, _filter(256, 256, 16, 16, 1, 320), R=64, nosplit=1),
    # (28 groups for each of the 192 early workgroups cover all 4096: nothing is left for the late ones)
    _v("16x128x128-ge28", 262144, 16384, _filter(256, 192, 28, 0, 0, 320), R=64, ge=28),
    _v("wgs-per-cu-2", 262144, 4096, _filter(512, 512, 8, 8, None, 512), wgs_per_cu=2),
    # (t_vq(8) = 13 us < 1.6 x 12 us: routers in front; delta = 11 groups, g_early = 12 covers everything)
    _v("wgs-per-cu-2-router", 262144, 4096, _filter(512, 448, 12, 0, 0, 576), R=64, wgs_per_cu=2),
    # ---- a router workgroup that needs more LDS than the VQ's: the launch takes the router's
    _v("router-lds-larger", 262144, 4096, _filter(256, 256, 16, 16, 1, 320, lds=70000), R=64, router_lds=70000),
    # ---- the exact loop: K without a filter path; the tile count by N (64 x ZT vectors per workgroup)
    _v("exact-65535", 65535, 4096, _exact(1, 1024, 1024, 20800, variant="plain"), K=1040),
    _v("exact-65536", 65536, 4096, _exact(2, 512, 512, 20800), K=1040),
    _v("exact-131071", 131071, 4096, _exact(2, 1024, 1024, 20800), K=1040),
    _v("exact-131072", 131072, 4096, _exact(4, 512, 512, 20800), K=1040),
    _v("exact-4194303", 4194303, 4096, _exact(4, 16384, 16384, 20800), K=1040),
    _v("exact-4194304", 4194304, 4096, _exact(8, 8192, 8192, 20800), K=1040),
    _v("exact-conv", 262144, 4096, dict(err=ERR_UNSUPPORTED, why="fused quant_conv needs K % 64 == 0 and K <= 1024"), K=1040, conv=1),
    _v("exact-knob", 262144, 4096, _exact(4, 1024, 1024, 20480, variant="plain"), exact=1),
    _v("exact-knob-router", 262144, 4096, _exact(4, 1024, 1088, ROUTER_LDS, variant="router"), exact=1, R=64, loss=1),
    _v("exact-knob-zt1", 262144, 4096, _exact(1, 4096, 4096, 20480), exact=1, zt=1),
]

# ---- router_plan: no refinement, the stand-alone launch's 96 KB unless a row says otherwise ---------------------------------------
R_DEFAULTS = dict(refine=0, has_scratch=0, scratch_bytes=0, queues=0, lds_budget=96 * 1024, lds_shared=LDS_SHARED, lds_refine=LDS_REFINE)
R_FIELDS = ("B", "h16", "w16", "c", "m", "per", "refine", "has_scratch", "scratch_bytes", "queues", "lds_budget", "lds_shared", "lds_refine")


def _r(name, B, h16, w16, c, m, per, want, **shape):
    return pytest.param("R", dict(R_DEFAULTS, B=B, h16=h16, w16=w16, c=c, m=m, per=per, **shape), want, id="router-" + name)


def _routed(mode, k_c, k_m, bands, wgs, **more):
    return dict(dict(mode=mode, k_c=k_c, k_m=k_m, bands=bands, wgs=wgs, nq=0, scratch_need=0), **more)


REFINED = dict(refine=1, lds_budget=78 * 1024)      # the fused launch with the pixels behind the maps
SCRATCH_64 = 64 * 24 * (256 + 1024)                 # 64 segments of 16x16: 24 bytes per coarse and medium patch

R_CASES = [
    _r("64x16x16", 64, 16, 16, 0.1, 0.8, 1, _routed(0, 26, 922, 1, 64, stage=1, lds=4096 + 32 + 5120)),
    _r("64x16x16-batch", 64, 16, 16, 0.1, 0.8, 0, _routed(0, 1638, 58982, 1, 1)),
    _r("8x48x48", 8, 48, 48, 0.1, 0.8, 1, _routed(0, 230, 8294, 8, 64)),
    _r("12x48x48-mode1", 12, 48, 48, 0, 0.5, 1, _routed(1, 0, 4608, 5, 60)),
    _r("1x32x32-mode2", 1, 32, 32, 0.5, 0, 1, _routed(2, 512, 0, 8, 8)),
    _r("40x32x32-mode3", 40, 32, 32, 0.3, 0.7, 1, _routed(3, 307, 0, 1, 40)),
    _r("1x85x128", 1, 85, 128, 0.1, 0.8, 1, _routed(0, 1088, 39168, 8, 8)),
    _r("3x5x7", 3, 5, 7, 0.1, 0.8, 1, _routed(0, 4, 126, 1, 3)),
    # the shapes tests/test_special_entropies.py routes on special values, one per path of the stand-alone launch: a 768x768 tile's row
    # bands (stage 1), a batch-global segment that stages only e8 (4096 + 640 + 16 x 5120 bytes), and two that stage nothing
    _r("specials-tile-row-bands", 1, 48, 48, 0.1, 0.8, 1, _routed(0, 230, 8294, 8, 8, stage=1, lds=4096 + 288 + 20 * 2304)),
    _r("specials-20x16x16-batch", 20, 16, 16, 0.1, 0.8, 0, _routed(0, 512, 18432, 1, 1, stage=2, lds=4096 + 640 + 16 * 5120)),
    _r("specials-32x16x16-batch", 32, 16, 16, 0.1, 0.8, 0, _routed(0, 819, 29491, 1, 1, stage=0, lds=4096 + 1024)),
    _r("specials-48x16x16-batch", 48, 16, 16, 0.1, 0.8, 0, _routed(0, 1229, 44237, 1, 1, stage=0, lds=4096 + 1536)),
    # round-half-even: the products are 0.5
    _r("1x2x2-half", 1, 2, 2, 0.125, 0.5, 1, _routed(0, 0, 10, 1, 1)),
    _r("1x1x1-half", 1, 1, 1, 0.5, 0.25, 1, _routed(0, 0, 3, 1, 1)),
    _r("mode4", 4, 16, 16, 1, 0, 1, _routed(4, 0, 0, 1, 4)),
    _r("mode5", 4, 16, 16, 0, 1, 1, _routed(5, 0, 0, 1, 4)),
    _r("mode6", 4, 16, 16, 0, 0, 1, _routed(6, 0, 0, 1, 4)),
    # modes 4-6 compare nothing: no refinement even with the pixels
    _r("mode4-pixels", 4, 16, 16, 1, 0, 1, _routed(4, 0, 0, 1, 4, refined=0, lds=4096 + 32 + 5120), **REFINED),
    _r("ratio-above-1", 1, 16, 16, 1.5, 0.2, 1, dict(err=ERR_INVALID, why="k out of range")),
    _r("2^29-coarse-patches", 1, 1 << 15, 1 << 14, 0.1, 0.8, 1, dict(err=ERR_UNSUPPORTED, why="segment too large")),
    # refinement: 4096 + 8 * ceil(N16 / 64) + 20 * N16 + 16 + 26264 bytes within 78 KB = 79872
    _r("refine-48x48-fits", 1, 48, 48, 0.1, 0.8, 1, _routed(0, 230, 8294, 8, 8, refined=1, stage=1, lds=76744), **REFINED),
    _r("refine-56x48-no-fit", 1, 56, 48, 0.1, 0.8, 1, dict(err=ERR_UNSUPPORTED, why="does not fit the LDS"), **REFINED),
    # ... in the stand-alone launch too: its 96 KB do not count for a refined segment
    _r("refine-56x48-no-fit-96k", 1, 56, 48, 0.1, 0.8, 1, dict(err=ERR_UNSUPPORTED, why="does not fit the LDS"), refine=1),
    # the refinement queues: two per segment when the caller wants them and gives a scratch
    _r("queues", 64, 16, 16, 0.1, 0.8, 1, _routed(0, 26, 922, 1, 64, nq=128, scratch_need=SCRATCH_64, refined=1, lds=ROUTER_LDS),
       has_scratch=1, scratch_bytes=SCRATCH_64, queues=1, **REFINED),
    _r("queues-no-scratch", 64, 16, 16, 0.1, 0.8, 1, _routed(0, 26, 922, 1, 64, refined=1), queues=1, **REFINED),
    # (without queues wanted: only the row bands of a segment exchange through them)
    _r("no-queues-wanted", 64, 16, 16, 0.1, 0.8, 1, _routed(0, 26, 922, 1, 64, refined=1), has_scratch=1, scratch_bytes=SCRATCH_64, **REFINED),
    _r("bands-take-queues", 1, 48, 48, 0.1, 0.8, 1, _routed(0, 230, 8294, 8, 8, nq=2, scratch_need=24 * 5 * 2304), has_scratch=1,
       scratch_bytes=24 * 5 * 2304, **REFINED),
    _r("queues-2049-segments", 2049, 16, 16, 0.1, 0.8, 1, _routed(0, 26, 922, 1, 2049, refined=1), has_scratch=1, scratch_bytes=1 << 40,
       queues=1, **REFINED),
    _r("scratch-one-byte-short", 64, 16, 16, 0.1, 0.8, 1, dict(err=ERR_INVALID, why="scratch too small"), has_scratch=1,
       scratch_bytes=SCRATCH_64 - 1, queues=1, **REFINED),
    # magic multipliers ceil(2^32 / d) of n8 = 1024, w8 = 32, n4 = 4096, w4 = 64 ...
    _r("magic", 64, 16, 16, 0.1, 0.8, 1, _routed(0, 26, 922, 1, 64, mg_n8=1 << 22, mg_w8=1 << 27, mg_n4=1 << 20, mg_w4=1 << 26)),
    # ... and 0 (divide) where (largest dividend) x (divisor) reaches 2^32: 65536 x 65536 and 262144 x 262144
    _r("magic-zero", 1, 128, 128, 0.1, 0.8, 1, _routed(0, 1638, 58982, 8, 8, mg_n8=0, mg_w8=1 << 24, mg_n4=0, mg_w4=1 << 23, stage=0, lds=6144)),
]
CASES = V_CASES + R_CASES
TEXT = ("path", "variant")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every case of the tables through ONE run of the compiled program: {case id: parsed output line}"""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp_path_factory.mktemp("encode_plan") / "encode_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", os.path.join(ROOT, "tests", "host", "encode_plan_main.cpp"), "-o", exe])
    text = "\n".join(" ".join([c.values[0]] + [str(c.values[1][f]) for f in (V_FIELDS if c.values[0] == "V" else R_FIELDS)])
                     for c in CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    parsed = {}
    for c, line in zip(CASES, out):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            kv = dict(t.split("=", 1) for t in line.split())
            parsed[c.id] = {k: v if k in TEXT else int(v) for k, v in kv.items()}
    return parsed


@pytest.mark.parametrize("kind,shape,want", CASES)
def test_encode_plan(plans, request, kind, shape, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got["err"] == want["err"] and want["why"] in got["why"]
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want
    if kind == "R":
        # ranks are k - 1, or 0; a launch with row bands stays within a quarter of the chip (every band must be resident)
        assert got["rank_c"] == max(got["k_c"] - 1, 0) and got["rank_m"] == max(got["k_m"] - 1, 0)
        assert got["wgs"] == got["nseg"] * got["bands"]
        if shape["per"] and got["bands"] > 1:
            assert got["wgs"] <= 64
        return
    assert got["grid"] == got["nblk"] + shape["R"]
    if got["path"] == "filter" and (got["g_late"] > 0 or got["n_early"] < got["nblk"]):
        # every group of 64 vectors is owned by a workgroup
        assert got["n_early"] * got["g_early"] + (got["nblk"] - got["n_early"]) * got["g_late"] >= -(-shape["N"] // 64)
