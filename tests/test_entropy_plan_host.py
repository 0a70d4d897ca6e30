"""The argument checks and the launch geometry of the entropy-map entry points (csrc/cgic_entropy_plan.h) without a GPU.  The header
is plain C++17: tests/host/entropy_plan_main.cpp is compiled with the host compiler alone and run over the cases below.  A workgroup
walks kEntWaves x ppw = 4 x 4 = 16 patches of a row band of 16 rows."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -2
BINS = np.linspace(-1.0, 1.0, 32, dtype=np.float32)            # what the package passes (entropy.py)
PPW = 4


def _bins(moved=None, by=0.0):
    b = BINS.copy()
    if moved is not None:
        b[moved] += np.float32(by)
    return " ".join(repr(float(v)) for v in b)


def _exp2_scale_bits(sigma):
    """the float64 expression of the host path, rounded to float32 once, as a bit pattern"""
    s = float(np.float32(sigma))
    return struct.unpack("<I", struct.pack("<f", np.float32(-0.5 * 1.4426950408889634 / (s * s))))[0]


def _grid(gx, gy, gz, sigma=0.01, nothing=0):
    return dict(nothing=nothing, gx=gx, gy=gy, gz=gz, exp2_scale_bits=_exp2_scale_bits(sigma))


def _refused(code, why):
    return dict(err=code, why=why)


CASES = [
    # ---- entropy_plan: H W images ppw sigma has_outputs ----
    pytest.param(f"plan 256 256 64 {PPW} 0.01 1", _grid(1, 16, 64), id="plan-64x256x256"),
    pytest.param(f"plan 16 16 1 {PPW} 0.01 1", _grid(1, 1, 1), id="plan-1x16x16"),
    pytest.param(f"plan 16 256 1 {PPW} 0.01 1", _grid(1, 1, 1), id="plan-width-256"),
    pytest.param(f"plan 16 272 1 {PPW} 0.01 1", _grid(2, 1, 1), id="plan-width-272"),
    pytest.param(f"plan 16 4096 1 {PPW} 0.01 1", _grid(16, 1, 1), id="plan-width-4096"),
    pytest.param(f"plan 768 768 6 {PPW} 0.01 1", _grid(3, 48, 6), id="plan-tiles-768x768-NT6"),
    pytest.param(f"plan 64 64 2 {PPW} 0.0105 1", _grid(1, 4, 2, sigma=0.0105), id="plan-sigma-0.0105"),
    pytest.param(f"plan 64 64 0 {PPW} 0.01 1", _grid(1, 4, 0, nothing=1), id="plan-no-images"),
    pytest.param(f"plan 64 64 2 {PPW} 0.01 0", _grid(1, 4, 2, nothing=1), id="plan-no-outputs"),
    # ---- the setup: nbins sigma window bins ----
    pytest.param(f"setup 32 0.01 2 {_bins()}", "ok", id="setup-reference"),
    pytest.param(f"setup 32 0.0105 5 {_bins()}", "ok", id="setup-sigma-0.0105"),
    pytest.param(f"setup 32 0.01 2 {_bins(7, 5e-6)}", "ok", id="setup-bin-moved-5e-6"),
    pytest.param(f"setup 31 0.01 2 {_bins()}", _refused(ERR_UNSUPPORTED, "entropy: nbins=31; the reference uses 32 (model.py:480)"), id="nbins-31"),
    pytest.param(f"setup 32 0 2 {_bins()}",
                 _refused(ERR_UNSUPPORTED, "entropy: sigma=0; the 2-bin window assumes the reference's sigma=0.01 (model.py:481)"), id="sigma-0"),
    pytest.param(f"setup 32 0.0106 2 {_bins()}",
                 _refused(ERR_UNSUPPORTED, "entropy: sigma=0.0106; the 2-bin window assumes the reference's sigma=0.01 (model.py:481)"),
                 id="sigma-0.0106"),
    pytest.param(f"setup 32 0.0106 5 {_bins()}",
                 _refused(ERR_UNSUPPORTED, "entropy: sigma=0.0106; the five-bin window assumes the reference's sigma=0.01 (model.py:481)"),
                 id="sigma-0.0106-five-bin"),
    pytest.param(f"setup 32 nan 2 {_bins()}", _refused(ERR_UNSUPPORTED, "entropy: sigma=nan"), id="sigma-nan"),
    pytest.param(f"setup 32 0.01 2 {_bins(7, 2e-5)}", _refused(ERR_UNSUPPORTED, "entropy: bins are not linspace(-1, 1, 32)"), id="bin-moved-2e-5"),
    pytest.param(f"setup 32 0.01 5 {_bins(31, -2e-5)}", _refused(ERR_UNSUPPORTED, "entropy: bins are not linspace(-1, 1, 32)"), id="last-bin-moved-2e-5"),
    pytest.param(f"setup 31 0 2 {_bins(7, 2e-5)}", _refused(ERR_UNSUPPORTED, "entropy: nbins=31"), id="nbins-before-sigma"),
    pytest.param(f"setup 32 0 2 {_bins(7, 2e-5)}", _refused(ERR_UNSUPPORTED, "entropy: sigma=0;"), id="sigma-before-bins"),
    # ---- the image form: B H W ----
    pytest.param("image 64 256 256", "ok", id="image-64x256x256"),
    pytest.param("image 0 16 16", "ok", id="image-empty-batch"),
    pytest.param("image 65535 16 16", "ok", id="image-B-65535"),
    pytest.param("image 1 24 32", _refused(ERR_INVALID, "entropy: H=24 W=32 must be positive multiples of 16"), id="image-H-24"),
    pytest.param("image 1 32 24", _refused(ERR_INVALID, "entropy: H=32 W=24 must be positive multiples of 16"), id="image-W-24"),
    pytest.param("image 1 0 16", _refused(ERR_INVALID, "entropy: H=0 W=16 must be positive multiples of 16"), id="image-H-0"),
    pytest.param("image -1 16 16", _refused(ERR_INVALID, "must be positive multiples of 16"), id="image-B-negative"),
    pytest.param("image 65536 16 16", _refused(ERR_UNSUPPORTED, "entropy: batch/height exceed the grid limits"), id="image-B-65536"),
    pytest.param(f"image 1 {16 * 65536} 16", _refused(ERR_UNSUPPORTED, "entropy: batch/height exceed the grid limits"), id="image-rows-65536"),
    # ---- the tiles form: N H W T th tw [origins] ----
    pytest.param("tiles 1 2040 1356 6 768 768 -132 -90 -132 678 636 -90 636 678 1404 -90 1404 678", "ok", id="tiles-2040x1356"),
    pytest.param("tiles 0 2040 1356 1 768 768", "ok", id="tiles-no-images"),
    pytest.param(f"tiles 1365 64 64 48 16 16 {' '.join(['0 0'] * 48)}", "ok", id="tiles-NT-65520"),
    pytest.param(f"tiles 1 64 64 1 16 16 {-(1 << 29) + 1} {(1 << 29) - 1}", "ok", id="tiles-origin-largest"),
    pytest.param("tiles 1 0 64 1 16 16", _refused(ERR_INVALID, "entropy_maps_tiles: bad source shape"), id="tiles-source-H-0"),
    pytest.param(f"tiles 1 64 {1 << 30} 1 16 16", _refused(ERR_INVALID, "entropy_maps_tiles: bad source shape"), id="tiles-source-W-2^30"),
    pytest.param("tiles 1 64 64 0 16 16",
                 _refused(ERR_UNSUPPORTED, "entropy_maps_tiles: 0 tiles per image in this group (1..48): cut them with cgic_cut_tiles"), id="tiles-T-0"),
    pytest.param("tiles 1 64 64 49 16 16",
                 _refused(ERR_UNSUPPORTED, "entropy_maps_tiles: 49 tiles per image in this group (1..48): cut them with cgic_cut_tiles"), id="tiles-T-49"),
    pytest.param("tiles 1 64 64 1 16 24", _refused(ERR_INVALID, "entropy_maps_tiles: tile 16x24 must be positive multiples of 16"), id="tiles-16x24"),
    pytest.param("tiles 16384 64 64 4 16 16", _refused(ERR_UNSUPPORTED, "entropy: batch/height exceed the grid limits"), id="tiles-NT-65536"),
    pytest.param(f"tiles 1 64 64 2 16 16 0 0 0 {1 << 29}", _refused(ERR_INVALID, "entropy_maps_tiles: tile origin out of range"), id="tiles-origin-2^29"),
    pytest.param(f"tiles 1 64 64 1 16 16 {-(1 << 29)} 0", _refused(ERR_INVALID, "entropy_maps_tiles: tile origin out of range"), id="tiles-origin-minus-2^29"),
    # the order of the checks: the source shape, the tile count, the tile shape, the grid limits
    pytest.param("tiles 1 0 64 0 16 24", _refused(ERR_INVALID, "bad source shape"), id="tiles-source-before-T"),
    pytest.param("tiles 65536 64 64 49 16 24", _refused(ERR_UNSUPPORTED, "49 tiles per image"), id="tiles-T-before-tile-shape"),
    pytest.param("tiles 65536 64 64 1 16 24", _refused(ERR_INVALID, "tile 16x24"), id="tiles-tile-shape-before-grid"),
]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every case through ONE run of the compiled program: {case id: parsed output line}"""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp_path_factory.mktemp("entropy_plan") / "entropy_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", os.path.join(ROOT, "tests", "host", "entropy_plan_main.cpp"), "-o", exe])
    text = "\n".join(c.values[0] for c in CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(CASES)
    parsed = {}
    for c, line in zip(CASES, out):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        elif line == "ok":
            parsed[c.id] = "ok"
        else:
            parsed[c.id] = {k: int(v) for k, v in (t.split("=", 1) for t in line.split())}
    return parsed


@pytest.mark.parametrize("case,want", CASES)
def test_entropy_plan(results, request, case, want):
    got = results[request.node.callspec.id]
    if isinstance(want, dict) and "err" in want:
        assert isinstance(got, dict) and got.get("err") == want["err"] and want["why"] in got["why"], got
    else:
        assert got == want
