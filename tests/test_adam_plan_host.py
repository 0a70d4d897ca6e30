"""The work list and the arithmetic of a cgic_adam_plan (csrc/cgic_adam_plan.h) without a GPU.  The header is plain C++17:
tests/host/adam_plan_main.cpp is compiled with the host compiler alone -- once plainly, once with -fsanitize=address,undefined -- and
run as a program over the tables below.  Plans (rows worked out by hand):
  chunk      4096 elements; a tensor of n elements has ceil(n / 4096) chunks, the last one n - 4096 (chunks - 1) long; none for n = 0;
  grid       min(chunks, 2048);
  chunks16   chunks of entries whose param, exp_avg, exp_avg_sq AND shadow (if any) are 16-byte aligned;
  table_bytes  64 (one omd per EMA group) + 16 * 16 (the groups) + 48 per entry + 16 per chunk + 8 per entry (step_size, bc2_sqrt) +
             8 per entry (the gradient's address) = 320 + 64 entries + 16 chunks.
The prologue (adam_scalars) and the element chain (adam_element, adam_shadow) -- the text host and device share -- are compared BIT FOR
BIT with tests/adam_ref.py; the power rule is also measured against Python's beta ** t (profiles/adam.md has the figures)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adam_ref as aref
import ema_ref as eref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
CHUNK = 4096
P, M, V, S, T = 1 << 36, 2 << 36, 3 << 36, 4 << 36, 5 << 36          # 64 GiB apart, 16-byte aligned
D, N = 6 << 36, (6 << 36) + 64
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ema.npz"))
MODEL_NUMEL = [int(n) for n in GOLDEN["model/numel"]]


def entries(sizes, dp=0, dm=0, dv=0, ds=0, group=-1):
    """consecutive tensors 1 MiB-aligned apart; group -1: no shadow"""
    out, at = [], 0
    for n in sizes:
        out.append((P + dp + at, M + dm + at, V + dv + at, S + ds + at if group >= 0 else 0, n, group))
        at += -(-max(n, 1) * 4 // (1 << 20)) * (1 << 20)
    return out


def plan_line(ents, groups=(), steps=T):
    return " ".join(["plan %d %d %d" % (len(ents), len(groups), steps)] + ["%d %d %d %d %d %d" % e for e in ents] + ["%d %d" % g for g in groups])


def case(name, line, want):
    return pytest.param(line, want, id=name)


def plan(ents, groups=(), chunks16=None, table=None):
    sizes = [e[4] for e in ents]
    chunks = sum(-(-n // CHUNK) for n in sizes)
    want = dict(entries=len(ents), elements=sum(sizes), chunks=chunks, chunk=CHUNK, grid=min(chunks, 2048), groups=len(groups),
                shadowed=sum(1 for e in ents if e[5] >= 0), table_bytes=320 + 64 * len(ents) + 16 * chunks, covered=1)
    if chunks16 is not None:
        want["chunks16"] = chunks16
    if table is not None:
        want["table"] = table
    return want


def err(why, code=INVALID):
    return dict(err=code, why=why)


G1, G2 = [(D, N)], [(D, N), (D + 128, 0)]
SIZES = (0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
TABLES = {0: "-", 1: "0:0:1", 3: "0:0:3", 4: "0:0:4", 5: "0:0:5", CHUNK - 1: "0:0:4095", CHUNK: "0:0:4096", CHUNK + 1: "0:0:4096,0:4096:1",
          2 * CHUNK + 3: "0:0:4096,0:4096:4096,0:8192:3"}
CASES = []
for n in SIZES:
    c = -(-n // CHUNK)
    CASES.append(case(f"one-tensor-of-{n}", plan_line(entries([n])), plan(entries([n]), (), c, TABLES[n])))
MANY = [1 + i % 7 for i in range(700)]
MIXED = entries([9, CHUNK + 1], group=0)[:1] + entries([9, CHUNK + 1])[1:] + [(P + (8 << 20), M + (8 << 20), V + (8 << 20), S + (8 << 20), 5, 1)]
SIXTEEN = [(D + 64 * i, N + 64 * i) for i in range(16)]
CASES += [
    # ---- worked by hand: 0 + 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 = 11 chunks, 20 496 elements, 320 + 9 * 64 + 11 * 16 = 1072 bytes
    case("all-sizes-in-one-plan", plan_line(entries(SIZES)),
         dict(plan(entries(SIZES), (), 11, "1:0:1,2:0:3,3:0:4,4:0:5,5:0:4095,6:0:4096,7:0:4096,7:4096:1,8:0:4096,8:4096:4096,8:8192:3"),
              chunks=11, elements=20496, table_bytes=1072, grid=11)),
    case("all-sizes-with-shadows", plan_line(entries(SIZES, group=0), G1), dict(plan(entries(SIZES, group=0), G1, 11), shadowed=9, groups=1, table_bytes=1072)),
    case("700-one-chunk-entries", plan_line(entries(MANY)), dict(plan(entries(MANY), (), 700, "-"), chunks=700, grid=700, table_bytes=320 + 64 * 700 + 16 * 700)),
    case("one-tensor-of-40-chunks-beside-them", plan_line(entries(MANY + [40 * CHUNK])), dict(plan(entries(MANY + [40 * CHUNK]), (), 740), chunks=740)),
    case("more-chunks-than-the-grid", plan_line(entries([2049 * CHUNK + 5])), dict(plan(entries([2049 * CHUNK + 5]), (), 2050), chunks=2050, grid=2048)),
    # ---- two groups, one entry in each, one entry in none: 1 + 2 + 1 chunks; the group of an entry is kept
    case("two-groups-and-an-entry-without", plan_line(MIXED, G2), dict(plan(MIXED, G2, 4, "0:0:9,1:0:4096,1:4096:1,2:0:5"), shadowed=2, groups=2)),
    case("sixteen-groups", plan_line(entries([5], group=15), SIXTEEN), dict(plan(entries([5], group=15), SIXTEEN, 1), groups=16)),
    # ---- alignment: any one operand 4 bytes off takes the entry's chunks off the 16-byte path; 8 bytes is no multiple of 16 either
    case("all-aligned", plan_line(entries([CHUNK + 1, 9], group=0), G1), plan(entries([CHUNK + 1, 9], group=0), G1, 3)),
    case("param-off-by-4", plan_line(entries([CHUNK + 1, 9], dp=4)), plan(entries([CHUNK + 1, 9], dp=4), (), 0)),
    case("exp-avg-off-by-4", plan_line(entries([CHUNK + 1, 9], dm=4)), plan(entries([CHUNK + 1, 9], dm=4), (), 0)),
    case("exp-avg-sq-off-by-8", plan_line(entries([CHUNK + 1, 9], dv=8)), plan(entries([CHUNK + 1, 9], dv=8), (), 0)),
    case("shadow-off-by-12", plan_line(entries([CHUNK + 1, 9], ds=12, group=0), G1), plan(entries([CHUNK + 1, 9], ds=12, group=0), G1, 0)),
    case("one-entry-off-its-neighbours-aligned", plan_line([(P, M, V, 0, 9, -1), (P + 4096, M + 4096 + 12, V + 4096, 0, 9, -1), (P + 8192, M + 8192, V + 8192, 0, 9, -1)]),
         plan([(P, M, V, 0, 9, -1), (P + 4096, M + 4096 + 12, V + 4096, 0, 9, -1), (P + 8192, M + 8192, V + 8192, 0, 9, -1)], (), 2, "0:0:9,1:0:9,2:0:9")),
    # ---- empty plans
    case("no-entries", plan_line([], (), 0), dict(plan([], (), 0, "-"), table_bytes=320, grid=0)),
    case("no-entries-but-a-group", plan_line([], G1, 0), dict(plan([], G1, 0, "-"), table_bytes=320, grid=0, groups=1)),
    case("no-entries-no-list", "null 0", dict(plan([], (), 0, "-"), table_bytes=320, grid=0)),
    case("only-empty-tensors", plan_line([(0, 0, 0, 0, 0, -1), (P, M, V, S, 0, 0)], G1), dict(plan([(0, 0, 0, 0, 0, -1), (P, M, V, S, 0, 0)], G1, 0, "-"), grid=0)),
    # ---- every refusal
    case("null-param", plan_line([(P, M, V, 0, 3, -1), (0, M + 64, V + 64, 0, 5, -1)]), err("adam_plan: entry 1 has a NULL param with 5 elements")),
    case("null-exp-avg", plan_line([(P, 0, V, 0, 5, -1)]), err("adam_plan: entry 0 has a NULL exp_avg with 5 elements")),
    case("null-exp-avg-sq", plan_line([(P, M, 0, 0, 5, -1)]), err("adam_plan: entry 0 has a NULL exp_avg_sq with 5 elements")),
    case("null-shadow-in-a-group", plan_line([(P, M, V, 0, 5, 0)], G1), err("adam_plan: entry 0 has a NULL shadow with 5 elements in EMA group 0")),
    case("shadow-without-a-group", plan_line([(P, M, V, S, 5, -1)], G1), err("adam_plan: entry 0 has a shadow but no EMA group")),
    case("param-off-by-2", plan_line([(P, M, V, 0, 3, -1), (P + 66, M + 64, V + 64, 0, 5, -1)]), err("adam_plan: the param of entry 1 is not aligned to its 4-byte element")),
    case("exp-avg-off-by-1", plan_line([(P, M + 1, V, 0, 3, -1)]), err("adam_plan: the exp_avg of entry 0 is not aligned to its 4-byte element")),
    case("exp-avg-sq-off-by-3", plan_line([(P, M, V + 3, 0, 3, -1)]), err("adam_plan: the exp_avg_sq of entry 0 is not aligned to its 4-byte element")),
    case("shadow-off-by-2", plan_line([(P, M, V, S + 2, 3, 0)], G1), err("adam_plan: the shadow of entry 0 is not aligned to its 4-byte element")),
    case("misaligned-empty-tensor", plan_line([(P, M + 1, V, 0, 0, -1)]), err("adam_plan: the exp_avg of entry 0 is not aligned to its 4-byte element")),
    case("negative-n", plan_line([(P, M, V, 0, 3, -1), (P + 64, M + 64, V + 64, 0, -1, -1)]), err("adam_plan: entry 1 has -1 elements")),
    case("group-out-of-range", plan_line([(P, M, V, S, 3, 1)], G1), err("adam_plan: entry 0 names EMA group 1 of 1 (-1: no shadow)")),
    case("group-with-no-groups", plan_line([(P, M, V, S, 3, 0)]), err("adam_plan: entry 0 names EMA group 0 of 0 (-1: no shadow)")),
    case("group-below-minus-one", plan_line([(P, M, V, 0, 3, -2)], G1), err("adam_plan: entry 0 names EMA group -2 of 1 (-1: no shadow)")),
    case("seventeen-groups", "groups 17", err("adam_plan: 17 EMA groups (0 .. 16)")),
    case("negative-groups", "groups -1", err("adam_plan: -1 EMA groups (0 .. 16)")),
    case("no-group-list", "nullgroups 2", err("adam_plan: NULL group list with 2 EMA groups")),
    case("null-decay", plan_line([], [(0, N)], 0), err("adam_plan: EMA group 0 has a NULL decay")),
    case("decay-off-by-2", plan_line([], [(D, N), (D + 2, 0)], 0), err("adam_plan: the decay of EMA group 1 is not aligned to its 4-byte element")),
    case("num-updates-off-by-1", plan_line([], [(D, N + 1)], 0), err("adam_plan: the num_updates of EMA group 0 is not aligned to its 4-byte element")),
    case("null-steps", plan_line([(P, M, V, 0, 3, -1)], (), 0), err("adam_plan: NULL step counts with 1 entries")),
    case("steps-off-by-2", plan_line([(P, M, V, 0, 3, -1)], (), T + 2), err("adam_plan: the step counts are not aligned to their 4-byte element")),
    case("negative-count", "count -1", err("adam_plan: -1 entries (0 .. 2^31 - 1: an entry index is an int32)")),
    case("count-beyond-int32", "count 2147483648", err("adam_plan: 2147483648 entries (0 .. 2^31 - 1: an entry index is an int32)")),
    case("no-list", "null 3", err("adam_plan: NULL entry list with 3 entries")),
    case("chunks-beyond-int32", plan_line([(P, M, V, 0, (1 << 31) * CHUNK, -1)]), err("adam_plan: more than 2^31 - 1 chunks of 4096 elements (a chunk index is an int32)")),
    case("chunks-beyond-int32-in-sum", plan_line([(P, M, V, 0, (1 << 30) * CHUNK, -1), (P, M, V, 0, (1 << 30) * CHUNK, -1)]),
         err("adam_plan: more than 2^31 - 1 chunks of 4096 elements (a chunk index is an int32)")),
    # ---- the tensors of the model at the training config (tests/golden/ema.npz), all in one EMA group
    case("the-model", plan_line(entries(MODEL_NUMEL, group=0), G1), dict(plan(entries(MODEL_NUMEL, group=0), G1), grid=2048, entries=655, shadowed=655)),
]

# ---- the prologue: the step count found (fp32), lr, beta1, beta2
BETAS = ((0.5, 0.9), (0.9, 0.999), (0.0, 0.0), (1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24))
COUNTS = (0, 1, 2, 9, 1000, (1 << 24) - 1)
PRO = [(float(c), lr, b1, b2) for c in COUNTS for b1, b2 in BETAS for lr in (5e-5, 1e-3)]
PRO += [(float(1 << 24), 5e-5, 0.5, 0.9), (-1.0, 5e-5, 0.5, 0.9), (2.5, 5e-5, 0.5, 0.9), (float("nan"), 5e-5, 0.5, 0.9), (float("inf"), 5e-5, 0.5, 0.9),
        (4294967040.0, 1e-3, 0.9, 0.999), (7.0, 0.0, 0.5, 0.9), (7.0, float(np.float32(3e-4)), 0.5, 0.9)]

# ---- the element chain: (g, p, m, v) values crossed with settings (beta1, beta2, eps, weight_decay, clip or None) at two step counts
NAN, INF = float("nan"), float("inf")
VALUES = [(0.25, 1.0, 0.1, 0.01), (-3.0, -1.0, 0.5, 4.0), (NAN, 1.0, 0.1, 0.01), (INF, 1.0, 0.1, 0.01), (-INF, 1.0, 0.1, 0.01), (1.0, 1.0, 0.0, 0.0),
          (0.0, 1.0, 0.0, 0.0), (-0.0, -0.0, -0.0, 0.0), (1e-45, 1.0, 1e-45, 1e-45), (-5e-39, 1e-38, 5e-39, 1e-40), (3e38, 1.0, 3e38, 3e38),
          (1.0, NAN, 0.0, 0.0), (1.0, 1.0, NAN, 1.0), (1.0, 1.0, 0.0, INF), (1.0, INF, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0), (-1.0, 1.0, 1.0, 1.0),
          (1.0000001, 1.0, 0.0, 0.0), (-1.0000001, 1.0, 0.0, 0.0), (2.0, 1.0, 0.0, 0.0), (-2.0, 1.0, 0.0, 0.0), (0.99999994, 3.0, 0.3, 0.7),
          (1e-6, 0.3, 1e-7, 1e-13), (1e2, -0.3, 50.0, 2e3), (1.1754944e-38, 1.1754944e-38, 1.1754944e-38, 1.1754944e-38)]
SETTINGS = [(0.5, 0.9, 1e-8, 0.0, None), (0.5, 0.9, 1e-8, 0.0, 1.0), (0.5, 0.9, 1e-8, 0.01, 1.0), (0.9, 0.999, 1e-8, 0.0, None), (0.9, 0.999, 0.0, 0.01, None),
            (0.5, 0.9, 0.0, 0.0, None), (0.0, 0.0, 1e-8, 0.0, 1.0), (0.3, 0.9, 1e-8, 0.0, 0.5), (0.5, 0.9, 1e-8, 0.0, INF)]
EL = [(vals, st, step) for vals in VALUES for st in SETTINGS for step in (1.0, 1000.0)]
SH = [(s, p, omd) for s, p in ((1.0, 0.5), (NAN, 1.0), (1.0, INF), (-0.0, 0.0), (1e-45, -1e-45), (3e38, -3e38)) for omd in (0.0, 1.0, 9.999275e-05, 0.8181818, NAN)]


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _lines():
    out = [c.values[0] for c in CASES]
    out += ["pro %d %s %s %s" % (_bits(s), float(lr).hex(), float(b1).hex(), float(b2).hex()) for s, lr, b1, b2 in PRO]
    for (g, p, m, v), (b1, b2, eps, wd, clip), step in EL:
        ss, bc = aref.scalars(step, 5e-5, b1, b2)
        out.append("el %d %d %d %d %d %d %s %s %s %s %s %d" % (_bits(g), _bits(p), _bits(m), _bits(v), _bits(ss), _bits(bc), float(b1).hex(), float(b2).hex(),
                                                             float(eps).hex(), float(wd).hex(), float(0.0 if clip is None else clip).hex(), clip is not None))
    out += ["sh %d %d %d" % (_bits(s), _bits(p), _bits(o)) for s, p, o in SH]
    return out


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "adam_plan_main.cpp"), "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], input="\n".join(_lines()) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES) + len(PRO) + len(EL) + len(SH)
    parsed = {}
    for c, line in zip(CASES, lines):
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed[c.id] = dict(err=int(code[4:]), why=why)
        else:
            parsed[c.id] = {k: (v if k == "table" else int(v)) for k, v in (t.split("=", 1) for t in line.split())}
    rest = [tuple(int(t.split("=")[1]) for t in line.split()) for line in lines[len(CASES):]]
    parsed["pro"], parsed["el"], parsed["sh"] = rest[:len(PRO)], rest[len(PRO):len(PRO) + len(EL)], rest[len(PRO) + len(EL):]
    return parsed


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("adam_plan"), [], "adam_plan_main"))


def test_the_table_has_no_two_rows_of_one_name():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("line,want", CASES)
def test_adam_plan(plans, request, line, want):
    got = plans[request.node.callspec.id]
    if "err" in want:
        assert got == want
        return
    assert "err" not in got, got
    assert {k: got[k] for k in want} == want, got


def test_the_model_is_655_tensors_all_covered(plans):
    got = plans["the-model"]
    assert len(MODEL_NUMEL) == 655 and got["elements"] == sum(MODEL_NUMEL) == 130358967
    assert got["chunks"] == sum(-(-n // CHUNK) for n in MODEL_NUMEL) == got["chunks16"] and got["covered"] == 1 and got["grid"] == 2048


def _same(bits, want):
    want = np.float32(want)
    return np.isnan(np.uint32(bits).view(np.float32)) if np.isnan(want) else bits == _bits(want)


def test_the_prologue_is_adam_refs_float64(plans):
    """step + 1 in fp32, the power by square-and-multiply, the division and the square root in float64, one rounding to fp32 each"""
    assert len(plans["pro"]) == len(PRO)
    for (s, lr, b1, b2), (nxt, ss, bc) in zip(PRO, plans["pro"]):
        want_next = aref.next_step(s)
        want_ss, want_bc = aref.scalars(want_next, lr, b1, b2)
        assert _same(nxt, want_next) and _same(ss, want_ss) and _same(bc, want_bc), (s, lr, b1, b2)
    by = {k: (np.uint32(ss).view(np.float32), np.uint32(bc).view(np.float32)) for k, (_, ss, bc) in zip(PRO, plans["pro"]) if k[0] == k[0]}
    # the first step at (0.5, 0.9): step_size = lr / 0.5, bc2_sqrt = sqrt(1 - 0.9); beta = 0: no correction at all
    assert by[0.0, 5e-5, 0.5, 0.9] == (np.float32(5e-5 / 0.5), np.float32((1.0 - 0.9) ** 0.5))
    assert by[0.0, 1e-3, 0.0, 0.0] == (np.float32(1e-3), np.float32(1.0)) == by[1000.0, 1e-3, 0.0, 0.0]
    assert by[1000.0, 5e-5, 0.5, 0.9] == (np.float32(5e-5), np.float32(1.0))                # 0.5^1001 and 0.9^1001 are below 2^-53
    assert by[float((1 << 24) - 1), 5e-5, 0.5, 0.9] == by[float(1 << 24), 5e-5, 0.5, 0.9]  # 2^24 + 1 is 2^24 in fp32: the count stays
    assert by[-1.0, 5e-5, 0.5, 0.9][0] == np.inf and by[-1.0, 5e-5, 0.5, 0.9][1] == 0       # a count of 0 after the step: lr / 0
    assert by[2.5, 5e-5, 0.5, 0.9] == by[2.0, 5e-5, 0.5, 0.9]                               # 3.5 is cut off to 3
    x2 = 0.9 * 0.9                                                                          # 13 = 0b1101: (x * x^4) * x^8
    x4 = x2 * x2
    assert aref.power(0.9, 13) == (0.9 * x4) * (x4 * x4) and aref.power(0.9, 0) == 1.0 and aref.power(0.9, 1) == 0.9


def test_the_element_chain_is_adam_refs_fp32(plans):
    assert len(plans["el"]) == len(EL) == len(VALUES) * len(SETTINGS) * 2
    for ((g, p, m, v), (b1, b2, eps, wd, clip), step), got in zip(EL, plans["el"]):
        ss, bc = aref.scalars(step, 5e-5, b1, b2)
        want = aref.element([g], [p], [m], [v], aref.consts(b1, b2, eps, wd, clip), ss, bc)
        assert all(_same(b, w[0]) for b, w in zip(got, want)), ((g, p, m, v), (b1, b2, eps, wd, clip), step, got, want)
    # a clip at and beyond the bound; v = 0 with eps = 0 and a zero gradient is 0 / 0
    k = aref.consts(0.5, 0.9, 1e-8, 0.0, 1.0)
    one = aref.element([1.0], [1.0], [0.0], [0.0], k, 1e-4, 0.3)
    assert all(np.array_equal(a, b) for a, b in zip(one, aref.element([2.0], [1.0], [0.0], [0.0], k, 1e-4, 0.3)))
    assert all(np.array_equal(a, b) for a, b in zip(one, aref.element([1.0000001], [1.0], [0.0], [0.0], k, 1e-4, 0.3)))
    assert np.isnan(aref.element([np.nan], [1.0], [0.0], [0.0], k, 1e-4, 0.3)[0][0])
    assert np.isnan(aref.element([0.0], [1.0], [0.0], [0.0], aref.consts(0.5, 0.9, 0.0, 0.0, None), 1e-4, 0.3)[0][0])
    assert aref.consts(0.5, 0.9, 0, 0, None)["lerp_low"] is False and aref.consts(0.9, 0.999, 0, 0, None)["lerp_low"] is True


def test_the_shadow_is_ema_refs_expression(plans):
    import torch
    for (s, p, omd), (got,) in zip(SH, plans["sh"]):
        want = aref.shadow([s], [p], omd)[0]
        assert _same(got, want)
        ref = eref.step(torch.tensor([s], dtype=torch.float32), torch.tensor([p], dtype=torch.float32), omd)[0].numpy()
        assert _same(got, ref)


def test_adam_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "adam_plan_main_san")
    assert _run(exe) == plans


def test_the_power_rule_against_pythons_pow():
    """square-and-multiply against Python's beta ** t (the C library's pow) for t = 1 .. 100 000: both are within an ulp or so of the true
    power in float64, and what reaches the kernel is ONE fp32 rounding of step_size and bc2_sqrt.  The largest relative difference of
    those two is below one fp32 ulp (2^-23); profiles/adam.md records the figures this prints"""
    worst = {}
    for beta in (0.5, 0.9, 0.999):
        ds = db = 0.0
        differ = 0
        for t in range(1, 100001):
            mine, theirs = aref.power(beta, t), beta ** t
            a, b = np.float32(5e-5 / (1.0 - mine)), np.float32(5e-5 / (1.0 - theirs))
            c, d = np.float32((1.0 - mine) ** 0.5), np.float32((1.0 - theirs) ** 0.5)
            differ += int(a != b) + int(c != d)
            ds, db = max(ds, abs(float(a) - float(b)) / float(b)), max(db, abs(float(c) - float(d)) / float(d))
        worst[beta] = (ds, db, differ)
        print(f"power rule, beta {beta}: largest relative difference of fp32 step_size {ds:.3e}, of bc2_sqrt {db:.3e}, values that differ {differ} of 200000")
    assert all(ds <= 2.0 ** -23 and db <= 2.0 ** -23 for ds, db, _ in worst.values()), worst
