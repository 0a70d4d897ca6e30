#!/usr/bin/env python3
"""Compare device code kernel by kernel across assembly files, for a refactor that MOVES kernels between translation units.

    tools/device_asm_per_kernel.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]

The .s files are what tools/device_asm_diff.sh keeps (`hipcc <the Makefile's FLAGS> --cuda-device-only -S`).  Every kernel symbol of
the old files must exist exactly once in the new files with the same text: its code (label to .Lfunc_end), its .amdhsa_kernel
descriptor block and its entry in the amdhsa.kernels metadata (VGPR / SGPR counts, private segment size, arguments).  What legitimately
differs is normalised as device_asm_diff.sh does: the per-file __hip_cuid_<hash>, and the ordinal of a function inside its file in
local labels (and with it the padding in front of a label's comment).  .file and .ident lines are dropped.  Exit status 0 when every kernel is identical and none is missing or new."""
import re
import sys


def norm(text):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    text = re.sub(r"\bL?BB[0-9]+_", "BB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)[0-9]+", r".Lfunc_\1", text)
    text = re.sub(r"[ \t]+;", " ;", text)          # a label's comment is padded to a column: the padding follows the ordinal's digits
    return "\n".join(l for l in text.split("\n") if not re.match(r"\s*\.(file|ident)\b", l))


def kernels(path):
    s = open(path).read()
    out = {}
    meta = {}
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", s, re.S | re.M)
    for entry in re.split(r"^  - (?=\.)", m.group(1) if m else "", flags=re.M)[1:]:
        meta[re.search(r"^\s*\.name:\s+(\S+)", entry, re.M).group(1)] = entry
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, re.M):
        body = re.search(r"^%s:.*?^\.Lfunc_end[0-9]+:" % re.escape(name), s, re.S | re.M).group(0)
        desc = re.search(r"^\s*\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % re.escape(name), s, re.S | re.M).group(0)
        out[name] = (norm(body), norm(desc), norm(meta[name]))
    return out


def main(argv):
    cut = argv.index("--")
    old, new = {}, {}
    for side, paths in ((old, argv[:cut]), (new, argv[cut + 1:])):
        for p in paths:
            for name, parts in kernels(p).items():
                assert name not in side, f"{name} twice on one side"
                side[name] = (p, parts)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only in the {'new' if name in new else 'old'} files")
            bad += 1
            continue
        (po, a), (pn, b) = old[name], new[name]
        diff = [what for what, x, y in zip(("code", "descriptor", "metadata"), a, b) if x != y]
        regs = dict(re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\d+)", b[2]))
        print(f"{name}: {'DIFFERS in ' + ', '.join(diff) if diff else 'identical'} ({a[0].count(chr(10)) + 1} lines; "
              f"vgpr {regs.get('vgpr_count')} sgpr {regs.get('sgpr_count')} private {regs.get('private_segment_fixed_size')}; {po} -> {pn})")
        bad += bool(diff)
    print(f"{len(old)} kernels in the old files, {len(new)} in the new, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
