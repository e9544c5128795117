#!/usr/bin/env python3
"""Are the kernels of two builds the same?  tools/kernel_diff.py OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]

Reads device assembly as `hipcc -save-temps=obj` writes it (<unit>-hip-amdgcn-amd-amdhsa-gfx950.s), cuts it into functions
(`name: ; @name` .. `.Lfunc_endN`), and compares per name the instruction text and the `.amdhsa_kernel` descriptor (registers,
LDS, scratch), with the basic-block label numbers normalised and `;` comments and blank lines stripped.  Prints the kernels that
are missing, extra, duplicated or different; exit status 1 if there is any.  For moves between translation units: the numbers of
the labels depend on a function's position in its file, nothing else may.
"""
import re
import sys

START = re.compile(r"^(\S+):\s*; @(\S+)\s*$")


def functions(paths):
    """{name: (text, descriptor)} of every function in the files, and the names met more than once"""
    out, dup = {}, []
    for path in paths:
        name, text, desc, in_desc = None, [], [], False
        for raw in open(path):
            m = START.match(raw)
            if m and m.group(1) == m.group(2):
                name, text, desc, in_desc = m.group(1), [], [], False
                continue
            if name is None:
                continue
            if raw.startswith(".Lfunc_end"):
                if name in out:
                    dup.append(name)
                out[name] = ("\n".join(text), "\n".join(desc))
                name = None
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", raw.split(";")[0]).strip()
            if line.startswith(".amdhsa_kernel"):
                in_desc = True
            if line:
                (desc if in_desc else text).append(line)
            if line.startswith(".end_amdhsa_kernel"):
                in_desc = False
    return out, dup


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        sys.exit(__doc__)
    cut = argv.index("--")
    (old, dup_old), (new, dup_new) = functions(argv[:cut]), functions(argv[cut + 1:])
    bad = 0
    for title, names in (("missing", sorted(set(old) - set(new))), ("extra", sorted(set(new) - set(old))),
                         ("duplicated in OLD", dup_old), ("duplicated in NEW", dup_new),
                         ("different text", sorted(n for n in old if n in new and old[n][0] != new[n][0])),
                         ("different descriptor", sorted(n for n in old if n in new and old[n][1] != new[n][1]))):
        for n in names:
            print(f"{title}: {n}")
        bad += len(names)
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
