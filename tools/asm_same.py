#!/usr/bin/env python3
"""tools/asm_same.py <old> <new> -- are the kernels of two sets of hipcc -S listings the same
machine code?  <old> and <new> are each a directory of .s files, or one .s file (`make asm`
writes one listing per kernel unit into build/).  Kernels are matched by demangled name,
whichever listing they sit in.  Per kernel it compares the instruction stream (comments and
directives dropped, local label numbers renumbered in order of appearance) and the
.amdhsa_next_free_vgpr / _sgpr, .amdhsa_group_segment_fixed_size and
.amdhsa_private_segment_fixed_size of its descriptor.  Prints the kernels that differ or exist
on one side only, then the counts; exit status 1 unless the sets are equal."""
import glob
import os
import re
import subprocess
import sys

DESC = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
        ".amdhsa_private_segment_fixed_size")
LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def listings(path):
    return sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]


def kernels(path):
    """{mangled name: (instruction lines, descriptor values)} of every kernel in the listings"""
    out = {}
    for f in listings(path):
        lines = open(f).read().splitlines()
        desc, cur = {}, None
        for l in lines:
            t = l.split()
            if t[:1] == [".amdhsa_kernel"]:
                cur = desc.setdefault(t[1], {})
            elif t[:1] == [".end_amdhsa_kernel"]:
                cur = None
            elif cur is not None and t and t[0] in DESC:
                cur[t[0]] = t[1]
        body, name = {}, None
        for l in lines:
            m = re.match(r"^(\w+):", l)
            if m and m.group(1) in desc:
                name = m.group(1)
                body[name] = []
                continue
            if name is None:
                continue
            if l.startswith(".Lfunc_end"):
                name = None
                continue
            t = l.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            body[name].append(t)
        for k in desc:
            if k in out:
                sys.exit(f"{k}: defined twice in {path}")
            out[k] = (renumber(body.get(k, [])), desc[k])
    return out


def renumber(lines):
    seen = {}
    return [LOCAL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), l) for l in lines]


def demangle(names):
    names = list(names)
    for tool in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    dm = demangle(set(old) | set(new))
    old = {dm[k]: v for k, v in old.items()}
    new = {dm[k]: v for k, v in new.items()}
    bad = 0
    for k in sorted(set(old) ^ set(new)):
        print(("only in old: " if k in old else "only in new: ") + k)
        bad += 1
    for k in sorted(set(old) & set(new)):
        (oi, od), (ni, nd) = old[k], new[k]
        why = []
        if od != nd:
            why.append(" ".join(f"{d[8:]} {od.get(d)}->{nd.get(d)}" for d in DESC if od.get(d) != nd.get(d)))
        if oi != ni:
            at = next((i for i, (a, b) in enumerate(zip(oi, ni)) if a != b), min(len(oi), len(ni)))
            why.append(f"instructions {len(oi)}->{len(ni)}, first difference at {at}")
        if why:
            print(f"differs: {k}: " + "; ".join(why))
            bad += 1
    groups = {}
    for k in new:
        g = re.sub(r"^(void )?(\(anonymous namespace\)::)?", "", k).split("<")[0].split("(")[0]
        groups[g] = groups.get(g, 0) + 1
    print("kernels: old %d, new %d (%s)" % (len(old), len(new),
                                            ", ".join(f"{g} {n}" for g, n in sorted(groups.items()))))
    print("instructions compared: %d" % sum(len(v[0]) for v in new.values()))
    print("differences: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
