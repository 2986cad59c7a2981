#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (hipcc -S --cuda-device-only output, no GPU needed).

A source move must leave every kernel as it was: same instruction sequence (label numbers and comments normalised),
same register, LDS, scratch and accumulator-offset figures of its kernel descriptor.  Kernels are matched by name with
the anonymous namespace ignored (plain_name), so a parameter type may leave it and a kernel may change files.

    hipcc <the Makefile's flags> -S --cuda-device-only a.hip -o old/a.s     # ... for every file of either side
    python tools/device_code_diff.py old/a.s old/b.s -- new/c.s new/d.s     # exit code 1 on any difference

--gone REGEX (before the files) names, by their mangled names, the kernels the change means to drop: those must be missing
from the new build -- one that is still there counts as a difference, and so does any other missing kernel.
"""
import re
import sys

FIGURES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
           ".amdhsa_private_segment_fixed_size", ".amdhsa_accum_offset")


def plain_name(mangled):
    """the mangled name without its anonymous-namespace component: `12_GLOBAL__N_1` goes, and a type that was nested in
    it, `NS_<n><identifier>E` (S_ = the namespace), reads like the same type at namespace scope, `<n><identifier>`"""
    def unnest(m):
        n = int(m.group(1))
        rest = m.group(2)
        return m.group(1) + rest[:n] + rest[n + 1:] if rest[n:n + 1] == "E" else m.group(0)
    s = mangled.replace("12_GLOBAL__N_1", "")
    return re.sub(r"NS_(\d+)(\w*)", unnest, s)


def kernels(paths):
    """-> {plain name: (instructions, descriptor figures)} over the files"""
    found = {}
    for path in paths:
        text = open(path).read()
        bodies, cur = {}, None
        for line in text.split("\n"):
            t = line.split(";")[0].strip()
            m = re.match(r"^(_Z\w+):$", t)
            if m:
                cur = bodies.setdefault(m.group(1), [])
            elif t.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and t and (not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:$", t)):   # (labels stay)
                cur.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
            desc = dict(l.split()[:2] for l in m.group(2).split("\n") if l.strip())
            name = plain_name(m.group(1))
            assert name not in found, f"{name}: more than one kernel of that name"
            found[name] = (bodies[m.group(1)], tuple(desc[k] for k in FIGURES))
    return found


def main():
    args = sys.argv[1:]
    gone = re.compile(args[1]) if args[0] == "--gone" else None
    args = args[2:] if gone else args
    cut = args.index("--")
    old, new = kernels(args[:cut]), kernels(args[cut + 1:])
    bad = dropped = 0
    for name in sorted(set(old) | set(new)):
        if gone and gone.search(name):
            if name in new:
                print("STILL in the new build: " + name)
                bad += 1
            dropped += name in old
        elif name not in old or name not in new:
            print(("MISSING in the new build: " if name in old else "EXTRA in the new build: ") + name)
            bad += 1
        elif old[name] != new[name]:
            what = "instructions" if old[name][0] != new[name][0] else "descriptor " + str((old[name][1], new[name][1]))
            print(f"DIFFERENT ({what}): {name}")
            bad += 1
    if gone:
        print(f"{dropped} kernels of the old build dropped as expected")
    print(f"{len(old)} kernels of the old build, {len(new)} of the new, {bad} missing, extra or different; "
          f"{sum(len(v[0]) for n, v in old.items() if n in new)} instructions compared")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
