"""The host side of the device container (csrc/cgic_container_plan.h, container.parse_header) without a GPU.
The plan header is plain C++17: tests/host/container_plan_main.cpp is compiled with the host compiler alone -- once plainly, once with
-fsanitize=address,undefined -- and run as a program over the table below, whose rows were worked out by hand:
  header bytes 12 + 44 E;  bound 12 + 44 E + 5 E max(slot);  workspace = align16(8 (n + 1)) x 2 + align16(8 n) + align16(4 n), n = 5 E;
  stage launches ceil(E / 64);  pack words = ceil(capacity / 16) - floor(header / 16);  unpack words = sum over the written streams of
  floor((len + 7) / 16) + 1;  copy blocks = min(ceil(words / 256), 2048).
parse_header is checked against container.unpack on hand-built blobs."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import control_gic_amd as cg
from control_gic_amd import container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED, ERR_CAPACITY = -1, -2, -5
NAMES = cg.STREAM_NAMES
# model.py:225-260: which streams each routing mode writes
MODE_SETS = {0: (0, 1, 2, 3, 4), 1: (1, 2, 4), 2: (0, 2, 3), 3: (0, 1, 3), 4: (0,), 5: (1,), 6: (2,)}


def _entry(mode, lens, image_id=0, y=0, x=0, height=64, width=64, seed=0):
    rng = np.random.default_rng(seed)
    return dict(image_id=image_id, y=y, x=x, height=height, width=width, mode=mode,
                streams={NAMES[s]: rng.integers(0, 256, n, dtype=np.uint8).tobytes() for s, n in zip(MODE_SETS[mode], lens)})


def _hex(entries):
    return container.pack(entries).hex()


TWO = [_entry(0, (3, 40, 0, 2, 34)), _entry(0, (17, 16, 15, 2, 8), image_id=1, seed=1)]      # 79 + 58 payload bytes behind 100 of headers

CASES = [
    # ---- header bytes: the payload starts at every fourth residue mod 16
    ("H 0", dict(header=12, residue=12)),
    ("H 1", dict(header=56, residue=8)),
    ("H 2", dict(header=100, residue=4)),
    ("H 3", dict(header=144, residue=0)),
    ("H 4", dict(header=188, residue=12)),
    ("H 65535", dict(header=2883552, residue=0)),
    # ---- the bound: two groups of different slot sizes -- every stream as long as the LARGER slot
    ("B 2 3 1024 4096", dict(bound=144 + 15 * 4096)),
    ("B 2 3 4096 1024", dict(bound=144 + 15 * 4096)),
    ("B 1 0 1024", dict(bound=12)),
    ("B 0 0", dict(bound=12)),
    # ---- the workspace: E = 2 -> n = 10: 96 + 96 + 80 + 48
    ("W 2", dict(ws=320, off=0, words=96, ptr=192, len=272)),
    ("W 0", dict(ws=32)),
    # ---- pack: header 100, capacity 1000 -> words 6 .. 62
    ("P 1 2 1000  3 1024 0  0 0 0 2", dict(header=100, streams=10, stage=1, words=57, blocks=1, ws=320)),
    ("P 2 3 100000  2 1024 0 1 4096 3  0 0 1 0 0 1", dict(header=144, streams=15, stage=1, words=6250 - 9, blocks=25)),
    ("P 1 0 12  3 1024 0", dict(header=12, streams=0, stage=0, words=0, blocks=0)),
    ("P 0 0 0", dict(header=12, stage=0, blocks=0)),
    ("P 1 65 4096  65 1024 0 " + " ".join(f"0 {i}" for i in range(65)), dict(header=2872, stage=2, words=256 - 179, blocks=1)),
    ("P 1 64 4096  64 1024 0 " + " ".join(f"0 {i}" for i in range(64)), dict(header=2828, stage=1)),
    ("P 1 65535 50000000  1 1024 0", dict(header=2883552, streams=327675, stage=1024, words=3125000 - 180222, blocks=2048)),
    # (a capacity that ends inside the headers: nothing to copy, the device reports the capacity code)
    ("P 1 2 50  3 1024 0  0 0 0 2", dict(header=100, words=0, blocks=0)),
    # ---- the limits are refused
    ("P 1 65536 100  1 1024 0", dict(err=ERR_INVALID, why="entries outside")),
    ("P 65 0 100  " + "1 1024 0 " * 65, dict(err=ERR_INVALID, why="groups outside")),
    ("P 0 1 100  0 0", dict(err=ERR_INVALID, why="groups outside")),
    ("P 1 1 1000  3 1024 0  0 3", dict(err=ERR_INVALID, why="index is outside its group")),
    ("P 1 1 1000  3 1024 0  0 -1", dict(err=ERR_INVALID, why="index is outside its group")),
    ("P 1 1 1000  3 1024 0  1 0", dict(err=ERR_INVALID, why="names a group outside")),
    ("P 1 1 1000  3 1000 0  0 0", dict(err=ERR_INVALID, why="slot no positive multiple of 16")),
    ("P 1 1 1000  3 1024 7  0 0", dict(err=ERR_INVALID, why="mode outside")),
    ("P 1 1 -1  3 1024 0  0 0", dict(err=ERR_INVALID, why="negative capacity")),
    # ---- unpack: the file is checked in full; words = sum of floor((len + 7) / 16) + 1:  (1 + 3 + 1 + 1 + 3) + (2 + 2 + 2 + 1 + 1)
    (f"U 1 2  2 1024 0  0 0 0 1  {_hex(TWO)}", dict(header=100, streams=10, stage=1, words=17, blocks=1)),
    (f"U 1 0  2 1024 0  {_hex([])}", dict(header=12, words=0, blocks=0)),
    (f"U 1 2  2 1024 0  0 0 0 1  {_hex(TWO)[:-2]}", dict(err=ERR_INVALID, why="not the blob's size")),
    (f"U 1 2  2 1024 0  0 0 0 1  {_hex(TWO)}00", dict(err=ERR_INVALID, why="not the blob's size")),
    (f"U 1 2  2 1024 0  0 0 0 1  {_hex(TWO)[:150]}", dict(err=ERR_INVALID, why="ends inside its headers")),
    (f"U 1 2  2 1024 0  0 0 0 1  58{_hex(TWO)[2:]}", dict(err=ERR_INVALID, why="magic")),
    (f"U 1 2  2 1024 0  0 0 0 1  {_hex(TWO)[:8]}02{_hex(TWO)[10:]}", dict(err=ERR_UNSUPPORTED, why="version")),
    (f"U 1 1  2 1024 0  0 0  {_hex(TWO)}", dict(err=ERR_INVALID, why="entry count")),
    (f"U 1 2  2 1024 1  0 0 0 1  {_hex(TWO)}", dict(err=ERR_INVALID, why="mode is not its group's")),
    (f"U 1 2  2 48 0  0 0 0 1  {_hex(TWO)}", dict(header=100, words=17)),                       # 40 + 8 <= 48
    (f"U 1 2  2 32 0  0 0 0 1  {_hex(TWO)}", dict(err=ERR_CAPACITY, why="does not fit its slot")),
    (f"U 1 1  1 1024 0  0 0  {_hex([dict(_entry(1, (4, 4, 4)), mode=0)])}", dict(err=ERR_INVALID, why="not the set its mode writes")),
    (f"U 1 1  1 1024 4  0 0  {container.pack([_entry(4, (5,))])[:36].hex()}feffffff{container.pack([_entry(4, (5,))])[40:].hex()}",
     dict(err=ERR_INVALID, why="length below -1")),
    ("U 1 0  1 1024 0  -", dict(err=ERR_INVALID, why="ends inside its headers")),
]


def _build(tmp, flags, name):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler found (the build needs one too)"
    exe = str(tmp / name)
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-O1", *flags, os.path.join(ROOT, "tests", "host", "container_plan_main.cpp"), "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], input="\n".join(c for c, _ in CASES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES)
    parsed = []
    for line in lines:
        if line.startswith("err="):
            code, why = line.split(" why=", 1)
            parsed.append(dict(err=int(code[4:]), why=why))
        else:
            parsed.append({k: int(v) for k, v in (t.split("=", 1) for t in line.split())})
    return parsed


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("container_plan"), [], "container_plan_main"))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}-" + c.split("  ")[0][:24].replace(" ", "_") for k, (c, _) in enumerate(CASES)])
def test_container_plan(plans, k):
    want, got = CASES[k][1], plans[k]
    if "err" in want:
        assert got.get("err") == want["err"] and want["why"] in got["why"], got
        return
    assert "err" not in got, got
    assert {key: got[key] for key in want} == want


def test_container_plan_under_address_and_undefined_sanitizers(tmp_path, plans):
    """the same program, instrumented, run as a program: the same answers and nothing reported (the blob of a `U` case is an exact-size
    heap block, so a read past a truncated file would be seen)"""
    exe = _build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "container_plan_main_san")
    assert _run(exe) == plans


# ---- parse_header against unpack ------------------------------------------------------------------------------------------------
def _check_against_unpack(entries):
    blob = container.pack(entries)
    back = container.unpack(blob)
    assert back == entries
    m = container.parse_header(blob)
    assert m["n_entries"] == len(entries) and m["payload_start"] == 12 + 44 * len(entries) and m["size"] == len(blob)
    assert m["lens"].shape == (len(entries), 5) and m["offsets"].shape == (len(entries), 5)
    for k, e in enumerate(back):
        assert [int(m[f][k]) for f in ("image_id", "y", "x", "height", "width", "mode")] == [e[f] for f in ("image_id", "y", "x", "height", "width", "mode")]
        for s, name in enumerate(NAMES):
            if name in e["streams"]:
                at, n = int(m["offsets"][k, s]), int(m["lens"][k, s])
                assert n == len(e["streams"][name]) and blob[at:at + n] == e["streams"][name]
            else:
                assert int(m["lens"][k, s]) == -1
    return blob, m


def test_parse_header_matches_unpack():
    blob, m = _check_against_unpack([])
    assert blob == struct.pack("<4sHHI", b"CGIC", 1, 0, 0) and m["lens"].size == 0
    # all seven modes' stream sets, one entry each, positions and ids that use the upper bits of the fields
    _check_against_unpack([_entry(mode, tuple(3 + 2 * i + mode for i in range(len(MODE_SETS[mode]))), image_id=mode + (1 << 31), y=768 * mode,
                                  x=(1 << 32) - 16, height=592, width=768, seed=mode) for mode in range(7)])
    # zero-length streams: offsets coincide
    _, m = _check_against_unpack([_entry(0, (0, 5, 0, 0, 2)), _entry(1, (0, 0, 0), image_id=1), _entry(4, (7,), image_id=2)])
    assert m["offsets"][0].tolist() == [144, 144, 149, 149, 149] and m["offsets"][1].tolist() == [151] * 5
    assert m["offsets"][2].tolist() == [151, 158, 158, 158, 158]


def test_parse_header_refuses_what_unpack_refuses_and_more():
    blob = container.pack(TWO)
    for bad in (blob[:-1], blob + b"\0", b"XXXX" + blob[4:], blob[:4] + b"\2" + blob[5:]):
        with pytest.raises(ValueError):
            container.unpack(bad)
        with pytest.raises(ValueError):
            container.parse_header(bad)
    for bad in (blob[:5], blob[:60], b""):                        # cut inside the header / the entry table
        with pytest.raises(ValueError):
            container.parse_header(bad)
    # a length below -1
    with pytest.raises(ValueError, match="below -1"):
        container.parse_header(blob[:36] + struct.pack("<i", -2) + blob[40:])
    # lengths that do not add up: one stream claims a byte more / a byte less than the payload holds
    for d in (1, -1):
        with pytest.raises(ValueError):
            container.parse_header(blob[:40] + struct.pack("<i", 40 + d) + blob[44:])


def test_abi_has_the_container():
    assert cg._lib.lib().cgic_abi_version() >= 15
    l = cg._lib.lib()
    assert l.cgic_container_workspace_bytes(2) == 320 and l.cgic_container_workspace_bytes(65536) == 0
    g = (cg._lib.ContainerGroup * 2)(cg._lib.ContainerGroup(None, None, 1, 1024, 0), cg._lib.ContainerGroup(None, None, 1, 4096, 0))
    assert l.cgic_container_bound(g, 2, 3) == 144 + 15 * 4096
    # the limits are refused by the library itself, before it looks at a pointer
    e = (cg._lib.ContainerEntry * 1)(cg._lib.ContainerEntry(0, 0, 0, 64, 64, 0, 1))
    with pytest.raises(cg.CgicError) as err:
        cg._lib.call("cgic_container_pack", g, 2, e, 1, None, 0, None, None, None)
    assert err.value.code == ERR_INVALID and "index is outside its group" in str(err.value)
