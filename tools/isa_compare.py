#!/usr/bin/env python3
"""Compare the instruction streams of the k_cast_w instantiations in two device assembly files of csrc/pt_traverse_wide.hip.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt \\
        -fno-gpu-flush-denormals-to-zero -fno-fast-math --cuda-device-only -S -x hip csrc/pt_traverse_wide.hip -Iinclude -o wide.s
  python tools/isa_compare.py before.s after.s

Other kernels of any source file: --kernel NAME (repeatable) pairs the kernels whose mangled name is gmupt::NAME with any parameter list
(the instantiations of a template by their mangled template arguments), e.g. for csrc/pt_kernels.hip:

  python tools/isa_compare.py --kernel k_clear --kernel k_logic --kernel k_material before.s after.s

Kernels are paired by their template arguments <STATS, REPS> (the mangled names differ once the ray-source policy is a template
parameter: only the StateIO instantiation of the new file is paired).  Bodies are compared after renumbering the local labels by first
appearance and dropping comments and blank lines; .vgpr_count / .sgpr_count / LDS and scratch sizes are compared from the metadata.
Exit status 0 when everything is identical.
"""
import re
import sys

KERNEL = re.compile(r"^(_ZN5gmupt8k_cast_wILb([01])ELi(\d+)E(NS_7StateIOE)?EEv\S*):(\s|$)")
META_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def named(names):
    """Matcher of the kernels gmupt::NAME for NAME in names: (line) -> (key, mangled name) or None."""
    pat = re.compile(r"^(_ZN5gmupt(\d+)(\w+?)E\S*):(\s|$)")

    def match(line):
        m = pat.match(line)
        if m and m.group(3)[:int(m.group(2))] in names and len(m.group(3)) >= int(m.group(2)):
            n = int(m.group(2))
            targs = m.group(1)[len("_ZN5gmupt") + len(m.group(2)) + n:]      # of a template: its mangled arguments keep the instantiations apart
            return m.group(3)[:n] + (" " + targs if targs.startswith("I") else ""), m.group(1)
        return None
    return match


def cast_w(line):
    m = KERNEL.match(line)
    if m and (m.group(4) or "QueryIO" not in m.group(1)):
        return (m.group(2) == "1", int(m.group(3))), m.group(1)
    return None


def kernels(path, match=cast_w):
    lines = open(path).read().splitlines()
    out = {}
    i = 0
    while i < len(lines):
        km = match(lines[i])
        if km:
            key, name = km
            body = []
            i += 1
            while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
                body.append(lines[i])
                i += 1
            out[key] = {"name": name, "body": normalise(body)}
        i += 1
    # metadata (the YAML note at the end): .name follows the keys of its kernel's map in alphabetical order
    text = "\n".join(lines)
    for block in re.split(r"\n  - \.", text)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", block)
        if not nm:
            continue
        for key, k in out.items():
            if k["name"] == nm.group(1):
                k["meta"] = {mk: (re.search(re.escape(mk) + r":\s+(\d+)", block).group(1) if re.search(re.escape(mk) + r":\s+(\d+)", block) else None) for mk in META_KEYS}
    return out


def normalise(body):
    labels = {}
    res = []
    for l in body:
        l = l.split(";")[0].rstrip()
        if not l.strip():
            continue
        for lab in re.findall(r"\.LBB\d+_\d+", l):
            labels.setdefault(lab, ".L%d" % len(labels))
        l = re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], l)
        l = re.sub(r"_ZN5gmupt\d+k_\w+?E\S*?(?=[@+\s,)]|$)", "KERNEL", l)
        res.append(l)
    return res


def main():
    args = sys.argv[1:]
    names = [args[i + 1] for i in range(len(args) - 1) if args[i] == "--kernel"]
    files = [a for i, a in enumerate(args) if a != "--kernel" and (i == 0 or args[i - 1] != "--kernel")]
    match = named(set(names)) if names else cast_w
    a, b = kernels(files[0], match), kernels(files[1], match)
    ok = bool(a) or not names
    if names and {k.split(" ")[0] for k in a} != set(names):
        print("kernels not found in %s: %s" % (files[0], sorted(set(names) - {k.split(" ")[0] for k in a}))); ok = False
    for key in sorted(a):
        if key not in b:
            print("%s: missing in %s" % (a[key]["name"], files[1])); ok = False; continue
        same = a[key]["body"] == b[key]["body"]
        meta_same = a[key].get("meta") == b[key].get("meta")
        label = key if names else "k_cast_w<%s, %d>" % ("true" if key[0] else "false", key[1])
        print("%s: %d lines, body %s, metadata %s %s" % (label, len(a[key]["body"]),
              "identical" if same else "DIFFERS", "identical" if meta_same else "DIFFERS", a[key].get("meta")))
        if not meta_same:
            print("   after:", b[key].get("meta"))
        if not same:
            import difflib
            for d in list(difflib.unified_diff(a[key]["body"], b[key]["body"], lineterm="", n=1))[:40]:
                print("   " + d)
        ok = ok and same and meta_same
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
