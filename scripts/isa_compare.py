"""Compare the device code of `hipcc --cuda-device-only -S` outputs kernel by kernel.

A source change meant to leave the shipped kernels untouched (pruning an unused variant, a comment,
moving kernels between translation units) is checked here without a GPU: every kernel's instruction
stream (the whole body up to its .Lfunc_end label, early exits included), with labels, comments and
trailing blanks stripped, must be identical, and so must its register, LDS and scratch figures
(.amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr, .amdhsa_group_segment_fixed_size,
.amdhsa_private_segment_fixed_size), all four of which every kernel must state.  Each side may be several
files, the translation units of one build:

    python scripts/isa_compare.py before.s after.s [after2.s ...]
    python scripts/isa_compare.py before1.s before2.s -- after1.s after2.s

A kernel whose only differences are v_add_* / v_mul_* instructions with their two source operands
exchanged (commutative: the same result) is listed as "swapped", with the positions, and does not
fail the comparison; any other difference does (exit status 1)."""
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(txt):
    """{kernel: [instruction lines]} of one assembly text: a kernel's whole body, from its symbol to
    its .Lfunc_endN label (a kernel with early exits holds several s_endpgm)"""
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', txt, re.M | re.S):
        body = re.split(r'^\s*\.amdhsa_kernel\b', m.group(2), 1, flags=re.M)[0]   # the descriptor: resources()
        body = re.sub(r';[^\n]*', '', body)
        body = re.sub(r'\.L\w+', 'L', body)
        out[m.group(1)] = [line.rstrip() for line in body.split("\n")]
    return out


def resources(txt):
    """{kernel: {figure: value}} from the kernel descriptors of one assembly text"""
    out = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel', txt, re.M | re.S):
        out[m.group(1)] = {k: v for k, v in re.findall(r'\.amdhsa_(\w+)\s+(\S+)', m.group(2)) if k in RESOURCES}
    return out


def side(texts):
    """the kernels and resource figures of one side's files together, and the kernels defined twice"""
    ks, rs, twice = {}, {}, []
    for txt in texts:
        k = kernels(txt)
        twice += [n for n in k if n in ks]
        ks.update(k)
        rs.update(resources(txt))
    return ks, rs, sorted(twice)


def swap_only(b, a):
    """[(position, before, after)] when the two streams differ only in exchanged source operands of
    commutative adds and multiplies; None when they differ in any other way"""
    if len(b) != len(a):
        return None
    found = []
    for i, (x, y) in enumerate(zip(b, a)):
        if x == y:
            continue
        tx, ty = x.replace(",", " ").split(), y.replace(",", " ").split()
        if (len(tx) == 4 and len(ty) == 4 and tx[0] == ty[0] and re.match(r'v_(add|mul)_', tx[0])
                and tx[1] == ty[1] and tx[2] == ty[3] and tx[3] == ty[2]):
            found.append((i, x.strip(), y.strip()))
        else:
            return None
    return found


def compare(before, after):
    """before, after: lists of assembly texts.  Returns the findings as a dict of lists."""
    bk, br, btwice = side(before)
    ak, ar, atwice = side(after)
    res = {"before": len(bk), "after": len(ak), "changed": [], "swapped": [], "resources": [], "missing": [],
           "removed": sorted(set(bk) - set(ak)), "new": sorted(set(ak) - set(bk)), "twice": btwice + atwice}
    for k in sorted(set(bk) & set(ak)):
        if bk[k] != ak[k]:
            sw = swap_only(bk[k], ak[k])
            if sw is None:
                res["changed"].append(k)
            else:
                res["swapped"].append((k, sw))
        if br.get(k) != ar.get(k):
            res["resources"].append((k, br.get(k), ar.get(k)))
    # a kernel without its descriptor, or a descriptor without one of the four figures, proves nothing
    for name, ks, rs in (("before", bk, br), ("after", ak, ar)):
        res["missing"] += [(name, k, f) for k in sorted(ks) for f in RESOURCES if f not in rs.get(k, {})]
    res["ok"] = not (res["changed"] or res["resources"] or res["removed"] or res["new"] or res["twice"]
                     or res["missing"])
    return res


def main(argv):
    if "--" in argv:
        i = argv.index("--")
        bfiles, afiles = argv[:i], argv[i + 1:]
    else:
        bfiles, afiles = argv[:1], argv[1:]
    if not bfiles or not afiles:
        print(__doc__)
        return 2
    res = compare([open(f).read() for f in bfiles], [open(f).read() for f in afiles])
    print(f"kernels: {res['before']} before, {res['after']} after; changed {len(res['changed'])}, "
          f"operands swapped {len(res['swapped'])}, resource figures differ {len(res['resources'])}")
    for k in res["changed"]:
        print("  changed:", k)
    for k, sw in res["swapped"]:
        print("  swapped:", k)
        for pos, x, y in sw:
            print(f"    instruction {pos}: {x}  ->  {y}")
    for k, b, a in res["resources"]:
        print("  resources:", k, b, "->", a)
    for name, k, f in res["missing"]:
        print(f"  no .amdhsa_{f} ({name}):", k)
    for k in res["removed"]:
        print("  removed:", k)
    for k in res["new"]:
        print("  new:", k)
    for k in res["twice"]:
        print("  defined twice on one side:", k)
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
