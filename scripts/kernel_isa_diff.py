#!/usr/bin/env python3
"""Do two builds of the library hold the same kernels?  Compares two gfx950 assembly files of the library's translation unit,
kernel by kernel: which exist only in the old file, which only in the new one, and which exist in both with different
instruction streams.  A refactor that claims "no kernel changed" runs this against its parent and keeps the output
(profiles/front_bits_retired/isa_identity.txt is one).  No GPU needed; each compile takes about two minutes.

The two files: HIPCC_FLAGS of gr_amps_amd/build.py without -fPIC -shared, plus --cuda-device-only -S, from the root of each tree:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function \\
        --cuda-device-only -S -Iinclude -Igr_amps_amd/csrc gr_amps_amd/csrc/amps_recc.hip -o old.s      (in the parent's tree)
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function \\
        --cuda-device-only -S -Iinclude -Igr_amps_amd/csrc gr_amps_amd/csrc/amps_recc.hip -o new.s      (in this tree)

  python scripts/kernel_isa_diff.py old.s new.s [--rename REGEX REPL] [--expect-removed NAME ...] [--expect-added NAME ...]

A kernel here is every function symbol of the file (the __global__ kernels and the few device functions kept out of line).  Its
stream is the lines between its label and its end marker -- instructions and the kernel descriptor (registers, LDS, scratch) --
without comments and empty lines, with local labels (.LBB..., .Ltmp...) numbered in order of appearance and the kernel's own
symbol replaced by a placeholder.  Whole streams are compared; no instruction is looked for.  Kernels are matched by demangled
name (c++filt; mangled names without it).  --rename is applied to the OLD file's names, for a change that moves names and should
move nothing else, such as a dropped template parameter.  Exit status 1 if any kernel changed, or was added or removed without
being listed in --expect-added / --expect-removed (names as printed, after the rename); 0 otherwise."""
import argparse
import re
import shutil
import subprocess
import sys

_FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LOCAL = re.compile(r"\.L[A-Za-z]+\d+(?:_\d+)?")


def kernels(text):
    """{mangled name: [normalised stream lines]} of one assembly file"""
    out, name, lines, labels = {}, None, None, None
    for raw in text.splitlines():
        m = _FUNC.match(raw)
        if m:
            name, lines = m.group(1), None
            continue
        if name is None:
            continue
        if lines is None:                         # waiting for the kernel's label
            if raw.split(";")[0].strip() == name + ":":
                lines, labels = [], {}
            continue
        if _END.match(raw):
            out[name], name = lines, None
            continue
        line = " ".join(raw.split(";")[0].split())
        if not line:
            continue
        line = _LOCAL.sub(lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), line)
        lines.append(line.replace(name, "<self>"))
    return out


def demangle(names):
    names = list(names)
    if not names or not shutil.which("c++filt"):
        return {n: n for n in names}
    got = subprocess.run(["c++filt"], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return dict(zip(names, got)) if len(got) == len(names) else {n: n for n in names}


def compare(old_text, new_text, rename=None):
    """(removed, added, changed, compared): sorted names; changed as (name, old line count, new line count); compared = kernels in both"""
    sides = []
    for text, ren in ((old_text, rename), (new_text, None)):
        ks = kernels(text)
        dm = demangle(ks)
        sides.append({(re.sub(ren[0], ren[1], dm[n]) if ren else dm[n]): s for n, s in ks.items()})
    old, new = sides
    both = sorted(set(old) & set(new))
    changed = [(n, len(old[n]), len(new[n])) for n in both if old[n] != new[n]]
    return sorted(set(old) - set(new)), sorted(set(new) - set(old)), changed, len(both)


def report(old_text, new_text, rename=None, expect_removed=(), expect_added=(), out=sys.stdout):
    """prints the comparison and returns the exit status"""
    removed, added, changed, compared = compare(old_text, new_text, rename)
    print("compared %d  changed %d  removed %d  added %d" % (compared, len(changed), len(removed), len(added)), file=out)
    bad = len(changed)
    for what, names, expected in (("removed", removed, set(expect_removed)), ("added", added, set(expect_added))):
        for n in names:
            print("%s%s: %s" % (what, "" if n in expected else " (NOT expected)", n), file=out)
            bad += n not in expected
        for n in sorted(expected - set(names)):
            print("expected %s, but is not: %s" % (what, n), file=out)
            bad += 1
    for n, a, b in changed:
        print("changed: %s  (%d -> %d lines)" % (n, a, b), file=out)
    return 1 if bad else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"), help="re.sub applied to the old file's demangled names")
    ap.add_argument("--expect-removed", nargs="*", default=[], metavar="NAME")
    ap.add_argument("--expect-added", nargs="*", default=[], metavar="NAME")
    a = ap.parse_args(argv)
    with open(a.old) as f, open(a.new) as g:
        return report(f.read(), g.read(), a.rename, a.expect_removed, a.expect_added)


if __name__ == "__main__":
    sys.exit(main())
