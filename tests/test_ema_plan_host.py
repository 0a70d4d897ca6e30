"""The work list of a cgic_ema_plan (csrc/cgic_ema_plan.h) without a GPU: every check of the entries, the chunk table, the 16-byte
chunks, the grid, the size of the device tables, and the decay rule the prologue kernel runs.  The header is plain C++17:
tests/host/ema_plan_main.cpp is compiled with the host compiler alone -- once plainly, once with -fsanitize=address,undefined -- and
run as a program over the table below, whose rows were worked out by hand:
  chunk      4096 elements; a tensor of n elements has ceil(n / 4096) chunks, the last one n - 4096 (chunks - 1) long; none for n = 0;
  grid       min(chunks, 2048);
  chunks16   chunks of entries whose shadow AND param are 16-byte aligned (a chunk starts 16 384 bytes times k into its tensor);
  chunks16_stash  chunks of entries whose param is;
  stash      every entry rounded up to a multiple of 4 elements;
  table_bytes  16 (the omd float, padded) + 32 per entry + 16 per chunk.
The program checks by a walk of its own that every element of every entry lies in exactly one chunk (covered=1)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ema_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
CHUNK = 4096
S, P = 1 << 36, 2 << 36               # 64 GiB apart, 16-byte aligned
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ema.npz"))
MODEL_NUMEL = [int(n) for n in GOLDEN["model/numel"]]


def entries(sizes, ds=0, dp=0):
    """consecutive tensors 1 MiB-aligned apart, shadow side from S + ds, param side from P + dp"""
    out, at = [], 0
    for n in sizes:
        out.append((S + ds + at, P + dp + at, n))
        at += -(-max(n, 1) * 4 // (1 << 20)) * (1 << 20)
    return out


def plan_line(ents):
    return "plan %d " % len(ents) + " ".join("%d %d %d" % e for e in ents)


def case(name, line, want):
    return pytest.param(line, want, id=name)


def plan(ents, chunks16=None, chunks16_stash=None, table=None):
    sizes = [n for _, _, n in ents]
    chunks = sum(-(-n // CHUNK) for n in sizes)
    want = dict(entries=len(ents), elements=sum(sizes), chunks=chunks, chunk=CHUNK, grid=min(chunks, 2048),
                table_bytes=16 + 32 * len(ents) + 16 * chunks, stash=sum(-(-n // 4) * 4 for n in sizes), covered=1)
    if chunks16 is not None:
        want["chunks16"] = chunks16
    if chunks16_stash is not None:
        want["chunks16_stash"] = chunks16_stash
    if table is not None:
        want["table"] = table
    return want


def err(why, code=INVALID):
    return dict(err=code, why=why)


SIZES = (0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
TABLES = {0: "-", 1: "0:0:1", 3: "0:0:3", 4: "0:0:4", 5: "0:0:5", CHUNK - 1: "0:0:4095", CHUNK: "0:0:4096", CHUNK + 1: "0:0:4096,0:4096:1",
          2 * CHUNK + 3: "0:0:4096,0:4096:4096,0:8192:3"}
CASES = []
for n in SIZES:
    c = -(-n // CHUNK)
    CASES.append(case(f"one-tensor-of-{n}", plan_line(entries([n])), plan(entries([n]), c, c, TABLES[n])))
MANY = [1 + i % 7 for i in range(700)]
CASES += [
    # ---- worked by hand: 0 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 = 11 chunks, 20 496 elements, a stash of 20 508, 16 + 9 * 32 + 11 * 16 = 480 bytes
    case("all-sizes-in-one-plan", plan_line(entries(SIZES)),
         dict(plan(entries(SIZES), 11, 11, "1:0:1,2:0:3,3:0:4,4:0:5,5:0:4095,6:0:4096,7:0:4096,7:4096:1,8:0:4096,8:4096:4096,8:8192:3"),
              chunks=11, elements=20496, stash=20508, table_bytes=480, grid=11)),
    case("700-one-chunk-entries", plan_line(entries(MANY)), dict(plan(entries(MANY), 700, 700, "-"), chunks=700, grid=700, table_bytes=33616, elements=2800)),
    case("one-tensor-of-40-chunks-beside-them", plan_line(entries(MANY + [40 * CHUNK])), dict(plan(entries(MANY + [40 * CHUNK]), 740, 740), chunks=740)),
    case("more-chunks-than-the-grid", plan_line(entries([2049 * CHUNK + 1])), dict(plan(entries([2049 * CHUNK + 1]), 2050, 2050), chunks=2050, grid=2048)),
    # ---- the four alignment combinations (and 8 bytes: a multiple of 4 that is no multiple of 16)
    case("both-aligned", plan_line(entries([CHUNK + 1, 9])), plan(entries([CHUNK + 1, 9]), 3, 3)),
    case("shadow-off-by-4", plan_line(entries([CHUNK + 1, 9], ds=4)), plan(entries([CHUNK + 1, 9], ds=4), 0, 3)),
    case("param-off-by-4", plan_line(entries([CHUNK + 1, 9], dp=4)), plan(entries([CHUNK + 1, 9], dp=4), 0, 0)),
    case("both-off-by-4", plan_line(entries([CHUNK + 1, 9], ds=4, dp=4)), plan(entries([CHUNK + 1, 9], ds=4, dp=4), 0, 0)),
    case("both-off-by-8", plan_line(entries([9], ds=8, dp=8)), plan(entries([9], ds=8, dp=8), 0, 0)),
    case("one-entry-off-its-neighbours-aligned", plan_line([(S, P, 9), (S + 4096 + 12, P + 4096, 9), (S + 8192, P + 8192, 9)]),
         plan([(S, P, 9), (S + 4096 + 12, P + 4096, 9), (S + 8192, P + 8192, 9)], 2, 3, "0:0:9,1:0:9,2:0:9")),
    # ---- empty plans
    case("no-entries", "plan 0", dict(plan([], 0, 0, "-"), table_bytes=16, grid=0)),
    case("no-entries-no-list", "null 0", dict(plan([], 0, 0, "-"), table_bytes=16, grid=0)),
    case("only-empty-tensors", plan_line([(0, 0, 0), (S, P, 0)]), dict(plan([(0, 0, 0), (S, P, 0)], 0, 0, "-"), table_bytes=80, grid=0)),
    # ---- every refusal
    case("null-shadow", plan_line([(S, P, 3), (0, P + 64, 5)]), err("ema_plan: entry 1 has a NULL shadow with 5 elements")),
    case("null-param", plan_line([(S, 0, 5)]), err("ema_plan: entry 0 has a NULL param with 5 elements")),
    case("shadow-off-by-2", plan_line([(S, P, 3), (S + 66, P + 64, 5)]), err("ema_plan: the shadow of entry 1 is not aligned to its 4-byte element")),
    case("param-off-by-1", plan_line([(S, P + 1, 3)]), err("ema_plan: the param of entry 0 is not aligned to its 4-byte element")),
    case("misaligned-empty-tensor", plan_line([(S, P + 1, 0)]), err("ema_plan: the param of entry 0 is not aligned to its 4-byte element")),
    case("negative-n", plan_line([(S, P, 3), (S + 64, P + 64, -1)]), err("ema_plan: entry 1 has -1 elements")),
    case("negative-count", "count -1", err("ema_plan: -1 entries (0 .. 2^31 - 1: an entry index is an int32)")),
    case("count-beyond-int32", "count 2147483648", err("ema_plan: 2147483648 entries (0 .. 2^31 - 1: an entry index is an int32)")),
    case("no-list", "null 3", err("ema_plan: NULL entry list with 3 entries")),
    case("chunks-beyond-int32", plan_line([(S, P, (1 << 31) * CHUNK)]), err("ema_plan: more than 2^31 - 1 chunks of 4096 elements (a chunk index is an int32)")),
    case("chunks-beyond-int32-in-sum", plan_line([(S, P, (1 << 30) * CHUNK), (S, P, (1 << 30) * CHUNK)]),
         err("ema_plan: more than 2^31 - 1 chunks of 4096 elements (a chunk index is an int32)")),
    # ---- the tensors of the model at the training config (tests/golden/ema.npz)
    case("the-model", plan_line(entries(MODEL_NUMEL)), dict(plan(entries(MODEL_NUMEL)), grid=2048, entries=655)),
]

# ---- the decay rule: decay (as fp32 bits), num_updates before the call, whether a counter is given
DECAYS = (0.0, 0.5, 0.9999, 1.0, float("nan"))
COUNTS = (-1, 0, 1, 8, 89990, 89991, (1 << 24) + 1, (1 << 31) - 2)
OMD = [(d, n, 1) for d in DECAYS for n in COUNTS] + [(d, 5, 0) for d in DECAYS]


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "ema_plan_main.cpp"), "-o", exe])
    return exe


def _run(exe):
    text = "\n".join([c.values[0] for c in CASES] + ["omd %d %d %d" % (_bits(d), n, has) for d, n, has in OMD]) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES) + len(OMD)
    parsed = {}
    for c, line in zip(CASES, lines):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            parsed[c.id] = {k: (v if k == "table" else int(v)) for k, v in (t.split("=", 1) for t in line.split())}
    parsed["omd"] = [tuple(int(t.split("=")[1]) for t in line.split()) for line in lines[len(CASES):]]
    return parsed


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("ema_plan"), [], "ema_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_ema_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_the_model_is_655_tensors_all_covered(plans):
    """130 358 967 elements: 31 chunks or more for the big convolutions, one for each of the 430 tensors of at most 512 elements"""
    got = plans["the-model"]
    assert len(MODEL_NUMEL) == 655 and got["elements"] == sum(MODEL_NUMEL) == 130358967
    assert got["chunks"] == sum(-(-n // CHUNK) for n in MODEL_NUMEL) and got["covered"] == 1 and got["grid"] == 2048
    assert got["chunks16"] == got["chunks"]                     # (these made-up tensors are all aligned)
    assert sum(1 for n in MODEL_NUMEL if n <= 512) == 430


def test_one_minus_decay_is_numpys_fp32(plans):
    """ema_one_minus_decay, the text the prologue kernel runs, against fp32 numpy (tests/ema_ref.py, which tests/test_ema_host.py pins
    to the real class): either side of the crossing with 0.9999, a counter beyond 2^24 and one whose 1 + n wraps"""
    assert len(plans["omd"]) == len(OMD)
    for (d, n, has), (omd_bits, nxt) in zip(OMD, plans["omd"]):
        want = eref.one_minus_decay(d, n if has else None)
        got = np.uint32(omd_bits).view(np.float32)
        if np.isnan(want):
            assert np.isnan(got), (d, n, has)
        else:
            assert omd_bits == _bits(want), (d, n, has, got, want)
        assert nxt == eref.next_count(n)
    by = {(d, n, has): np.uint32(b).view(np.float32) for (d, n, has), (b, _) in zip(OMD, plans["omd"]) if d == d}
    one = np.float32(1.0)
    assert by[0.9999, -1, 1] == one - np.float32(0.9999) == by[0.9999, 5, 0]
    assert by[0.9999, 0, 1] == one - np.float32(2.0) / np.float32(11.0)                    # the counter becomes 1: 2 / 11
    assert by[0.9999, 8, 1] == one - np.float32(10.0) / np.float32(19.0)
    # the counter becomes 89 991: 89 992 / 90 001 = 0.99990000111 is not below the decay, which stays; likewise one step on
    assert by[0.9999, 89990, 1] == by[0.9999, 89991, 1] == one - np.float32(0.9999)
    assert np.float32(89992.0) / np.float32(90001.0) >= np.float32(0.9999) > np.float32(80000.0) / np.float32(80009.0)
    assert by[1.0, (1 << 31) - 2, 1] == 0.0 and by[0.5, (1 << 31) - 2, 1] == 0.5          # -2^31 / (-2^31 + 9) is 1.0 in fp32
    assert by[0.0, 0, 1] == 1.0 and by[1.0, -1, 1] == 0.0


def test_ema_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ema_plan_main_san")
    assert _run(exe) == plans
