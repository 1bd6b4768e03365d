"""Compare the register / scratch / LDS use of every kernel of one HIP source between two builds, from the compiler's
`-Rpass-analysis=kernel-resource-usage` remarks — no GPU needed.  Used to show that a compile-time flag added to a
shared walker did not leak into the instantiations that do not set it (the masked gather_fm).

    git show <parent commit>:recsys-benchmark_amd/csrc/gather_fm.hip > parent_gather_fm.hip
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Irecsys-benchmark_amd/csrc \
          -Rpass-analysis=kernel-resource-usage -c parent_gather_fm.hip -o parent.o 2> parent.txt
    hipcc (same flags) -c recsys-benchmark_amd/csrc/gather_fm.hip -o this.o 2> this.txt
    python tools/kernel_resource_diff.py parent.txt this.txt

Kernels are matched by their DEMANGLED name (an empty template parameter pack changes the mangled one only); a plain kernel
that the second build turned into a template on one bool flag is matched with its `<false>` instantiation ("AS" line).  Prints
every kernel of the first build whose VGPR, SGPR, AGPR, scratch, LDS or occupancy figure moved or that is gone, then a
count per kernel family; exit status 1 if anything moved.

`--as OLD=NEW` (repeatable) follows a kernel family that was renamed and gained trailing template parameters — a walker
moved into a header and parametrised by a policy: every kernel of the first build in family OLD is compared with EVERY
kernel of the second build in family NEW whose template arguments begin with OLD's (one line per policy).

    python tools/kernel_resource_diff.py parent.txt this.txt --as k_sparse_adam=mi::k_rows_pass \
        --as k_sparse_adam_long=mi::k_rows_join --as k_sparse_adam_anyD=mi::k_rows_any
"""
import re
import subprocess
import sys

KEYS = ["VGPRs", "TotalSGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        text = m.group(1).strip()
        name = re.match(r"Function Name: (\S+)", text)
        if name:
            cur = out.setdefault(name.group(1), {})
            continue
        field = re.match(r"(.+?):\s*(\S+)$", text)
        if field and cur is not None:
            cur[field.group(1).strip()] = field.group(2)
    names = sorted(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.replace("(anonymous namespace)::", ""): out[n] for n, d in zip(names, plain)}


def family(name):
    return re.sub(r"[<(].*", "", re.sub(r"^void ", "", name))


def renamed(name, b):
    """A plain kernel of the first build that became a template on ONE bool flag in the second (k<false> keeps the old body,
    possibly behind more parameters): the second build's only `family<false>(...)`, or None."""
    if "<" in family(name) or re.match(r"^(void )?[\w:]+<", name):
        return None
    hits = [n for n in b if re.sub(r"^void ", "", n).startswith(family(name) + "<false>(")]
    return hits[0] if len(hits) == 1 else None


def template_args(name):
    m = re.match(r"^(?:void )?[\w:]+<(.*)>\(", name)
    return m.group(1) if m else ""


def followed(name, b, renames):
    """The second build's kernels of the family `--as` maps this kernel's family to, with its template arguments in front."""
    new = renames.get(family(name))
    if new is None:
        return []
    args = template_args(name)
    return [n for n in sorted(b) if family(n) == new and (not args or template_args(n).startswith(args + ", "))]


def main():
    argv, renames = [], {}
    it = iter(sys.argv[1:])
    for arg in it:
        if arg == "--as":
            old, new = next(it).split("=", 1)
            renames[old] = new
        else:
            argv.append(arg)
    a, b = parse(argv[0]), parse(argv[1])
    fam, moved = {}, 0
    for name in sorted(a):
        f = fam.setdefault(family(name), [0, 0])
        f[0] += 1
        others = [] if name in b else followed(name, b, renames)
        if others:
            any_moved = False
            for other in others:
                d = [(k, a[name].get(k), b[other].get(k)) for k in KEYS if a[name].get(k) != b[other].get(k)]
                print("AS   ", name, "->", other, d if d else "unchanged")
                any_moved |= bool(d)
            f[1] += any_moved
            moved += any_moved
            continue
        other = name if name in b else renamed(name, b)
        if other is None:
            print("GONE ", name)
        else:
            d = [(k, a[name].get(k), b[other].get(k)) for k in KEYS if a[name].get(k) != b[other].get(k)]
            if other != name:
                print("AS   ", name, "->", other)
            if not d:
                continue
            print("MOVED", name, d)
        f[1] += 1
        moved += 1
    print(f"{len(a)} kernels in the first build: {len(a) - moved} unchanged, {moved} moved or gone; "
          f"{len(set(b) - set(a))} kernels only in the second build")
    for f, (n, m) in sorted(fam.items()):
        print(f"  {f}: {n} instantiations, {m} moved")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
