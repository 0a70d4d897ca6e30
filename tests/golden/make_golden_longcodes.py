#!/usr/bin/env python3
"""Golden fixture for code tables whose longest code has 14 to 65 bits (tests/golden/long_codes.npz), from the REAL reference
coder.

Runs only in the build container (needs /root/reference).  For every ladder table of tests/long_codes_ref.py (FIXTURE_TABLES:
1024 symbols with a longest code of 14, 32, 33, 63, 64 and 65 bits, 2560 symbols with 64) it builds the reference's own
`HuffmanCoding` (CGIC/tools/indices_coding.py) from a ParameterDict of the counts, and stores the counts, the code lengths, the
code words (MSB first, 1, 2 or 3 words of 32 bits) and the bytes the reference writes for the streams of
long_codes_ref.fixture_streams: none, 1, 2 and 65 symbols, and 1024 symbols of every content class.  Before it writes it
requires that the oracle (oracle/cgic_oracle.c) gives the same table and bytes, and that the reference decodes its own files.
Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_longcodes.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from CGIC.tools.indices_coding import HuffmanCoding  # noqa: E402

import long_codes_ref as lc  # noqa: E402
from oracle import cgic_oracle as orc  # noqa: E402


def check(cond, msg):
    if not cond:
        raise SystemExit("MISMATCH: " + msg)


def as_param_dict(counts):
    # the container type the reference hands HuffmanCoding (inference.py:137-139); float64, so that counts up to 2^53 stay exact
    return torch.nn.ParameterDict({str(i): torch.nn.Parameter(torch.tensor([float(v)], dtype=torch.float64))
                                   for i, v in enumerate(counts)}).requires_grad_(False)


def codes_to_arrays(h):
    n = len(h.codes)
    lens = np.array([len(h.codes[i]) for i in range(n)], np.int32)
    code = np.zeros((n, max(1, (int(lens.max()) + 31) // 32)), np.uint32)
    for i in range(n):
        for b, ch in enumerate(h.codes[i]):
            if ch == "1":
                code[i, b // 32] |= np.uint32(1 << (31 - b % 32))
    return lens, code


def main():
    out = {"tables": np.array(lc.FIXTURE_TABLES, np.int64)}
    for K, max_len in lc.FIXTURE_TABLES:
        counts = lc.ladder_table(K, max_len)
        pd = as_param_dict(counts)
        check([int(k) for k in pd.keys()] == lc.push_order(K), "ParameterDict key order")
        h = HuffmanCoding(pd)
        lens, code = codes_to_arrays(h)
        check(int(lens.max()) == max_len, f"K={K}: longest code {lens.max()}, wanted {max_len}")
        t = orc.HuffmanTable(counts)
        check(np.array_equal(t.len, lens), f"K={K} max_len={max_len}: oracle lengths")
        check(t.words == code.shape[1] and np.array_equal(t.code, code), f"K={K} max_len={max_len}: oracle codes")
        key = f"k{K}_l{max_len}"
        out[key + "_counts"], out[key + "_len"], out[key + "_code"] = counts, lens.astype(np.uint8), code
        for name, sym in lc.fixture_streams(lens):
            with tempfile.TemporaryDirectory() as d:
                p = h.compress(torch.from_numpy(sym), os.path.join(d, "s.bin"))
                data = open(p, "rb").read()
                dec = h.decompress_string(p)
            check((dec is None and len(sym) == 0) or dec == sym.tolist(), f"{key} {name}: the reference does not decode its own file")
            check(orc.encode(t, sym) == data, f"{key} {name}: oracle bytes")
            odec = orc.decode(t, data)
            check((odec is None and len(sym) == 0) or np.array_equal(odec, sym), f"{key} {name}: oracle decode")
            out[f"{key}_{name}_sym"] = sym.astype(np.int16)
            out[f"{key}_{name}_bytes"] = np.frombuffer(data, np.uint8)
        print(f"  {key}: {code.shape[1]} word(s), {int((lens > 13).sum())} codes beyond 13 bits, {int((lens > 32).sum())} beyond 32, "
              f"largest count 2^{np.log2(float(counts.max())):.2f} ok")
    path = os.path.join(HERE, "long_codes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote long_codes.npz ({os.path.getsize(path)} bytes); the oracle agrees with the reference on every table and stream")


if __name__ == "__main__":
    main()
