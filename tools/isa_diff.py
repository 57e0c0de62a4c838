#!/usr/bin/env python3
"""Are two builds of a kernel the same instruction stream?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude \
        --cuda-device-only -S conflux_amd/csrc/kernels.hip -o new.s
    python tools/isa_diff.py old.s new.s k_dgemm_f64_w8='k_dgemm_mfma<GemmW8>' \
        k_dgemm_f64_glds

Each pair is OLD=NEW (or one name for both).  A name is a mangled symbol, or
source-level identifiers (`kernel`, `kernel<Type>`) that must all occur in
exactly one kernel's mangled symbol.  Per pair: the text from the kernel's
label to its .Lfunc_end (instructions and kernel descriptor), comments
dropped, with local label numbers, the symbol itself, section directives and
the kernel-argument segment size normalised, is compared line by line;
the resource fields of the code-object metadata are printed for both.  Exits
non-zero when any pair differs in a line or a field.
"""
import difflib
import re
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size")


def find_symbol(text, name):
    syms = re.findall(r"^\t\.amdhsa_kernel (\S+)$", text, re.M)
    if name in syms:
        return name
    ids = re.findall(r"[A-Za-z_]\w*", name)   # Itanium: <length><identifier>
    hits = [s for s in syms
            if all(re.search(r"(?<!\d)%d%s" % (len(i), i), s) for i in ids)]
    if len(hits) != 1:
        sys.exit("%r matches %d kernels: %s" % (name, len(hits), hits))
    return hits[0]


def body(text, sym):
    m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(sym), text,
                  re.M | re.S)
    out = []
    for line in m.group(0).splitlines():
        line = line.split(";")[0].rstrip().replace(sym, "SYM")
        line = re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", line)
        # the range includes the kernel descriptor: an empty trailing kernel
        # parameter may change the argument segment's size and nothing else
        if line and not line.lstrip().startswith(
                (".section", ".text", ".amdhsa_kernarg_size")):
            out.append(line)
    return out


def resources(text, sym):
    block = re.search(r"^  - \.agpr_count:(?:(?!^  - ).)*?^    \.name: +%s$"
                      r"(?:(?!^  - ).)*" % re.escape(sym), text, re.M | re.S)
    return {f: int(re.search(r"^    \%s: +(\d+)" % f, block.group(0),
                             re.M).group(1)) for f in FIELDS}


def main(old_path, new_path, pairs):
    old, new = open(old_path).read(), open(new_path).read()
    bad = 0
    for pair in pairs:
        a, _, b = pair.partition("=")
        sa, sb = find_symbol(old, a), find_symbol(new, b or a)
        la, lb = body(old, sa), body(new, sb)
        ndiff = sum(1 for d in difflib.ndiff(la, lb) if d[0] in "+-")
        ra, rb = resources(old, sa), resources(new, sb)
        print("%s -> %s: %d / %d lines, %d differ" %
              (a, b or a, len(la), len(lb), ndiff))
        for f in FIELDS:
            print("    %-28s %6d %6d%s" %
                  (f, ra[f], rb[f], "" if ra[f] == rb[f] else "   DIFFERS"))
        bad += ndiff != 0 or ra != rb
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
