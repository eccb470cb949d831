"""Compare hipcc assembly function by function (labels normalised, comments dropped) and kernel by kernel in the `.amdhsa_`
descriptor (VGPRs, SGPRs, accum offset, LDS, scratch, and every other line of it): the check that a source refactor or an
added variant left the code AND the resources of the existing kernels untouched.  Exit status 1 on any difference, or on a
function, kernel or file that one side lacks.
usage: scripts/isa_all.sh old_dir   (on the old tree)    scripts/isa_all.sh new_dir   (on the new tree)
       python scripts/isa_diff.py old_dir new_dir        every *.s of both directories, paired by name, a report per file
       python scripts/isa_diff.py old.s new.s            one pair of files
       ... --rename OLD=NEW                              (repeatable) a kernel whose mangled name changed on purpose is compared
                                                         under its new name; a kernarg size that differs is reported, not counted"""
import os
import re
import sys

RESOURCES = (      # the descriptor lines that decide occupancy, named in the report
    "next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def funcs(path):
    """{function: [instruction lines]}, {kernel: {resource: value}}"""
    out, res, cur, kern, is_func = {}, {}, None, None, set()
    for line in open(path).read().split("\n"):
        m = re.match(r"\s*\.type\s+(_Z\w+),@function", line)
        if m:
            is_func.add(m.group(1))
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kern = m.group(1)
            res[kern] = {}
            continue
        if kern:                            # the descriptor sits inside the function: reported apart from its instructions
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", line)
            if m:
                res[kern][m.group(1)] = m.group(2)
            if re.match(r"\s*\.end_amdhsa_kernel", line):
                kern = None
            continue
        m = re.match(r"^(_Z\w+):", line)
        if m and m.group(1) in is_func:     # (not a data object: its "body" would run on to the end of the file)
            cur = m.group(1)
            out[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur:
            t = re.sub(r"\.LBB\d+_\d+", ".L", line.split(";")[0].rstrip())
            if t.strip():
                out[cur].append(t)
    return out, res


RENAMES = {}


def diff_files(pa, pb):
    (a, ra), (b, rb) = funcs(pa), funcs(pb)
    bad = 0
    for old, new in RENAMES.items():
        if old in a and new in b:
            print(f"{'renamed':10s} {old}\n{'':10s} -> {new}")
            a = {new if k == old else k: ([t.replace(old, new) for t in v] if k == old else v) for k, v in a.items()}
            ra[new] = ra.pop(old)
            if ra[new].get("kernarg_size") != rb[new].get("kernarg_size"):
                print(f"{'':10s} kernarg_size: {ra[new].get('kernarg_size')} -> {rb[new].get('kernarg_size')} (allowed under --rename)")
                ra[new]["kernarg_size"] = rb[new].get("kernarg_size")
    for k in a:
        same = a[k] == b.get(k)
        bad += not same
        print(f"{'identical' if same else ('MISSING' if k not in b else 'DIFFERENT'):10s} {len(a[k]):6d} lines  {k[:100]}")
    for k in b:
        if k not in a:
            bad += 1
            print(f"{'NEW':10s} {len(b[k]):6d} lines  {k[:100]}")
    for k in sorted(set(ra) | set(rb)):
        if k not in ra or k not in rb:
            bad += 1
            print(f"{'resources':10s} {'MISSING' if k not in rb else 'NEW'}  {k[:100]}")
        elif ra[k] != rb[k]:
            bad += 1
            print(f"{'resources':10s} DIFFERENT  {k[:100]}")
            for r in sorted(set(ra[k]) | set(rb[k])):
                if ra[k].get(r) != rb[k].get(r):
                    print(f"{'':10s} {r}: {ra[k].get(r)} -> {rb[k].get(r)}")
    print(f"{'resources':10s} of {len(ra)} kernels compared: every .amdhsa_ line ({', '.join(RESOURCES)}, ...)")
    return bad, len(a), len(ra)


def main(pa, pb):
    if not (os.path.isdir(pa) and os.path.isdir(pb)):
        return 1 if diff_files(pa, pb)[0] else 0
    names = lambda d: {f for f in os.listdir(d) if f.endswith(".s")}
    na, nb = names(pa), names(pb)
    bad = n_funcs = n_kernels = 0
    for f in sorted(na | nb):
        print(f"== {f}")
        if f not in na or f not in nb:
            bad += 1
            print(f"{'MISSING' if f not in nb else 'NEW':10s} file")
            continue
        b, nf, nk = diff_files(os.path.join(pa, f), os.path.join(pb, f))
        if not nf:      # (a source that failed to compile leaves no assembly behind)
            b += 1
            print(f"{'EMPTY':10s} file")
        bad, n_funcs, n_kernels = bad + b, n_funcs + nf, n_kernels + nk
    print(f"== {len(na | nb)} files, {n_funcs} functions, {n_kernels} kernels: "
          f"{'all identical in instructions and resources' if not bad else f'{bad} DIFFERENCES'}")
    return 1 if bad else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    while "--rename" in argv:
        i = argv.index("--rename")
        old, new = argv[i + 1].split("=")
        RENAMES[old] = new
        del argv[i:i + 2]
    sys.exit(main(argv[0], argv[1]))
