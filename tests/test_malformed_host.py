"""CPU: the oracle's verdict on malformed streams, pinned to the REAL reference (tests/golden/malformed.npz, written by
tests/golden/make_golden_malformed.py from the catalogue of tests/malformed_ref.py), and the catalogue itself: no mutation class is
vacuous, the overflow and extension lengths respect the slot the library computes, and the closed list of cases where the library is
stricter than the reference is worked out from the streams alone.  What tests/test_malformed_streams.py then demands of the GPU
decoders is the oracle's verdict; the decoder path of each of its cases is a row of tests/test_decode_plan_host.py."""
import collections
import functools

import numpy as np
import pytest

import long_codes_ref as lc
import malformed_ref as mr


@functools.lru_cache(maxsize=None)
def _zipf():
    from conftest import load_golden
    from oracle import cgic_oracle as orc
    orc.build()
    return orc.HuffmanTable(load_golden("coders")["zipf_freq"])


@functools.lru_cache(maxsize=None)
def _catalogues():
    """[(h, w, [Mutant])] of the fixture's grids"""
    from oracle import cgic_oracle as orc
    return [(h, w, mr.catalogue(orc, _zipf(), h, w, seed)) for (h, w), seed in zip(mr.FIXTURE_GRIDS, mr.FIXTURE_SEEDS)]


def _slice(blob, off, i):
    return blob[off[i]:off[i + 1]].tobytes()


def test_oracle_equals_the_reference_on_every_mutant(orc, golden):
    """raise or not, the decoded index grid and the three masks, for every mutant of the fixture: orc.decompress_image restates what
    the real CGIC.compress does with the mutated files -- an empty mask file raises, one decoded symbol is broadcast over the cells of
    its mask, a cell both coarse and medium carries -1 in the fine mask and in the sum"""
    g = golden("malformed")
    names = g["names"].tolist()
    i = io = mo = 0
    accepted = refused = 0
    for h, w, cat in _catalogues():
        n, nm = h * w, h * w // 16 + h * w // 4 + h * w
        for m in cat:
            assert names[i] == f"{h}x{w}-{m.name}" and int(g["mode"][i]) == m.mode and tuple(g["hw"][i]) == (h, w)
            for s, name in enumerate(orc.STREAM_NAMES):              # the fixture was made from these very bytes
                assert bool(g["present"][i, s]) == (name in m.streams), names[i]
                assert _slice(g["bytes"], g["bytes_off"], 5 * i + s) == m.streams.get(name, b""), (names[i], name)
            got = mr.verdict(orc, m, _zipf())
            assert (got is None) == bool(g["raised"][i]), (names[i], str(g["exc"][i]))
            if got is None:
                refused += 1
            else:
                accepted += 1
                assert np.array_equal(got[0], g["ind"][io:io + n].reshape(h, w)), names[i]
                assert np.array_equal(np.concatenate([a.ravel() for a in got[1:]]), g["masks"][mo:mo + nm]), names[i]
                io, mo = io + n, mo + nm
            i += 1
    assert i == len(names) and io == len(g["ind"]) and mo == len(g["masks"])
    assert accepted >= 150 and refused >= 250
    # a missing file is the one refusal that is no RuntimeError in the reference
    assert set(g["exc"][g["raised"]].tolist()) == {"RuntimeError", "FileNotFoundError"}
    assert all(("missing" in n) == (e == "FileNotFoundError") for n, e, r in zip(names, g["exc"].tolist(), g["raised"]) if r)


def test_oracle_single_stream_decode_equals_the_reference(orc, golden):
    """orc.decode == HuffmanCoding / BinaryCoding .decompress_string on every single-stream mutant (None for the empty file)"""
    g = golden("malformed")
    tabs = {"huffman": _zipf(), "binary": orc.HuffmanTable.binary()}
    want_names = [f"{h}x{w}-{name}" for (h, w), seed in zip(mr.FIXTURE_GRIDS, mr.FIXTURE_SEEDS)
                  for name, _, _ in mr.single_stream_mutants(orc, _zipf(), h, w, seed)]
    assert g["ss_names"].tolist() == want_names
    for i, kind in enumerate(g["ss_kind"].tolist()):
        got = orc.decode(tabs[kind], _slice(g["ss_bytes"], g["ss_bytes_off"], i))
        assert (got is None) == bool(g["ss_none"][i]), want_names[i]
        if got is not None:
            assert np.array_equal(got, g["ss_syms"][g["ss_syms_off"][i]:g["ss_syms_off"][i + 1]]), want_names[i]
    assert g["ss_none"].sum() >= 2 and set(g["ss_kind"].tolist()) == {"huffman", "binary"}


def _outcomes(orc, cat, htab):
    """{(class, 'index' | 'mask'): Counter of 'refused' | 'same' | 'diff'} of a catalogue, against the clean decode of the mode"""
    clean = {m.mode: mr.verdict(orc, m, htab) for m in cat[:3]}
    assert all(v is not None for v in clean.values())
    out = collections.defaultdict(collections.Counter)
    for m in cat[3:]:
        v = mr.verdict(orc, m, htab)
        kind = "refused" if v is None else "same" if all(np.array_equal(a, b) for a, b in zip(v, clean[m.mode])) else "diff"
        out[(m.cls, "mask" if m.kind in mr.MASK_STREAMS else "index")][kind] += 1
    return out


def test_no_class_is_vacuous(orc):
    """on the oracle alone, over the fixture's grids: every class where both outcomes are possible holds a mutant that is accepted with
    a result other than the clean decode (or, where the text can only lose an incomplete tail, the clean one) and one that is refused;
    every other class has the one outcome that defines it"""
    tot = collections.defaultdict(collections.Counter)
    for h, w, cat in _catalogues():
        for k, v in _outcomes(orc, cat, _zipf()).items():
            tot[k].update(v)
    # both outcomes
    for k in (("empty", "index"), ("flip", "index"), ("header", "index"), ("truncate", "index"), ("one_bit", "mask")):
        assert tot[k]["diff"] >= 1 and tot[k]["refused"] >= 1, (k, dict(tot[k]))
    # trailing bytes under the old header: refused when they hold a codeword, accepted (the incomplete code is dropped) when not
    assert tot[("extend_keep", "index")]["same"] >= 1 and tot[("extend_keep", "index")]["refused"] >= 1
    assert tot[("header", "index")]["same"] >= 1                      # one pad bit less: a bit that completes no code
    # the last symbol is lost: refused, unless ONE symbol is left, which the reference broadcasts
    assert tot[("cut_codeword", "index")]["refused"] >= 1 and tot[("cut_codeword", "index")]["same"] == 0
    # one outcome
    for k, only in ((("extend_adjust", "index"), "same"), (("empty_valid", "index"), "same"), (("noncanonical", "mask"), "same"),
                    (("flip_keep", "index"), "diff"), (("two_bits", "mask"), "diff"), (("overlap", "mask"), "diff"),
                    (("flip_change", "index"), "refused"), (("overflow", "index"), "refused"),
                    (("swap", "index"), "refused"), (("length", "mask"), "refused"), (("mask_header", "mask"), "refused"),
                    (("missing", "index"), "refused"), (("missing", "mask"), "refused")):
        assert tot[k][only] >= 1 and set(tot[k]) == {only}, (k, dict(tot[k]))
    assert {c for c, _ in tot} == {"empty", "empty_valid", "truncate", "extend_keep", "extend_adjust", "header", "cut_codeword", "flip", "flip_keep",
                                   "flip_change", "overflow", "swap", "length", "mask_header", "noncanonical", "one_bit", "two_bits", "overlap", "missing"}


def test_overflow_and_text_unchanged_mutants_are_what_they_claim(orc):
    htab = _zipf()
    for h, w, cat in _catalogues():
        clean = {m.mode: m for m in cat[:3]}
        seen = collections.Counter()
        for m in cat[3:]:
            if m.cls == "overflow":
                cap = {"indices_coarse": h * w // 16, "indices_medium": h * w // 4, "indices_fine": h * w}[m.kind]
                assert len(orc.decode(htab, m.streams[m.kind])) > 4 * cap, m.name
            elif m.cls in mr.TEXT_UNCHANGED:
                assert np.array_equal(orc.decode(htab, m.streams[m.kind]), orc.decode(htab, clean[m.mode].streams[m.kind])), m.name
                assert len(m.streams[m.kind]) > len(clean[m.mode].streams[m.kind])
            elif m.cls == "cut_codeword":
                assert len(orc.decode(htab, m.streams[m.kind])) == len(orc.decode(htab, clean[m.mode].streams[m.kind])) - 1, m.name
            seen[m.cls] += 1
        assert seen["overflow"] >= 5 and seen["extend_adjust"] >= 25 and seen["cut_codeword"] >= 5


def test_the_stricter_list_is_closed_and_worked_out_from_the_streams(orc):
    """the three cases where the library refuses what the reference accepts: every non-canonical mask and every overlap mutant is
    one, the broadcasts are found by their one decoded symbol, and nothing that the oracle refuses, nor a clean image, is listed"""
    htab = _zipf()
    found = collections.Counter()
    for h, w, cat in _catalogues():
        for m in cat:
            why = mr.stricter(orc, m, htab)
            assert why is None or why in mr.STRICTER
            if m.cls == "clean":
                assert why is None
            if m.cls == "noncanonical":
                assert why == "noncanonical_mask"
            if m.cls == "overlap":
                assert why == "overlap"
            if why is not None:
                assert mr.verdict(orc, m, htab) is not None or why == "noncanonical_mask", m.name
                found[why] += 1
    assert set(found) == set(mr.STRICTER), found


class _V:
    def __init__(self, v): self.v = v
    def item(self): return self.v


def _native_table(counts):
    import control_gic_amd as cg
    return cg.HuffmanCoding({str(s): _V(float(counts[s])) for s in lc.push_order(len(counts))}).table


@pytest.mark.parametrize("table,h,w", sorted({(t, h, w) for t, _, h, w, _ in mr.GPU_CASES}, key=str), ids=str)
def test_lengths_respect_the_library_slot(orc, golden, table, h, w):
    """slot_bytes restates cgic_compress_slot_bytes for every table and grid of the GPU cases; the table's (symbols, longest code) is
    what the plan rows assume; and for the small grids the whole catalogue is built: len + 8 <= slot for every stream of it"""
    from control_gic_amd import _lib
    counts = golden("coders")["zipf_freq"] if table == "zipf" else np.array(mr.TWO_COUNTS) if table == "two" else lc.ladder_table(*table)
    tab = _native_table(counts)
    assert (len(counts), tab.max_len) == mr.table_shape(table)
    slot = int(_lib.lib().cgic_compress_slot_bytes(tab.handle, h, w))
    assert slot == mr.slot_bytes(tab.max_len, h, w)
    if h * w <= 32 * 48:
        htab = orc.HuffmanTable(counts)
        cat = mr.catalogue(orc, htab, h, w, seed=h * w, slot=slot)
        # the overflow mutants fill the slot up to its 8 bytes of slack, within one codeword and the pad
        assert slot - 8 - 2 <= max(len(d) for m in cat for d in m.streams.values()) <= slot - 8
        classes = {m.cls for m in cat}
        assert {"overflow", "extend_keep", "extend_adjust", "truncate", "header", "flip", "length", "missing"} <= classes
