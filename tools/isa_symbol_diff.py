"""Per-kernel companion of tools/isa_identity.sh for a unit that GAINED kernels: the whole-file diff is then never empty, and the order in
which the compiler emits the instantiations may move.  Splits the two stripped assembly files the script left in its workdir into
functions (from `.type NAME,@function` to the matching `.size NAME`) and into the per-kernel `.amdhsa_kernel` / metadata blocks, and
compares them symbol by symbol.  Local labels carry the function's position in the unit (.LBB12_5, .Lfunc_end12); the position is
replaced by `N` and trailing comments are dropped before comparing:

    bash tools/isa_identity.sh /tmp/parent /tmp/isa norm; python tools/isa_symbol_diff.py /tmp/isa/parent/norm.s /tmp/isa/new/norm.s

One line per class (identical / changed / only in the parent / only in the new tree), the names of everything but the identical ones,
exit status 1 if a symbol of the parent changed or vanished."""
import re
import sys


LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = LOCAL.sub(r".L\1N", line.split(";")[0].rstrip() + "\n")  # (trailing comments name the loop header's label)
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"\s*\.size\s+%s\b" % re.escape(name), line):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def descriptors(path):
    """.amdhsa_kernel NAME ... .end_amdhsa_kernel: registers, LDS, scratch as the loader sees them"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name, body = m.group(1), []
        elif name is not None:
            if ".end_amdhsa_kernel" in line:
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def main():
    a, b = sys.argv[1:3]
    bad = 0
    for what, split in (("code", functions), ("descriptor", descriptors)):
        pa, pb = split(a), split(b)
        same = [k for k in pa if k in pb and pa[k] == pb[k]]
        changed = [k for k in pa if k in pb and pa[k] != pb[k]]
        gone = [k for k in pa if k not in pb]
        new = [k for k in pb if k not in pa]
        print("%s: %d identical, %d changed, %d only in the parent, %d only in the new tree" % (what, len(same), len(changed), len(gone), len(new)))
        for tag, ks in (("changed", changed), ("only in the parent", gone), ("only in the new tree", new)):
            for k in ks:
                print("  %s: %s" % (tag, k))
        bad |= bool(changed or gone)
    return bad


if __name__ == "__main__":
    sys.exit(main())
