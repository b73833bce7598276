"""Per-kernel register table of two builds, and the twin check of a new kernel kind.

Build the library twice with the compiler's resource remarks on stderr,

    make -C cglb_amd/csrc clean all EXTRA_DEFS=-Rpass-analysis=kernel-resource-usage 2> after.log

(the same for the commit before the change: before.log), then

    python tools/resource_usage_table.py before.log after.log [--all] > profiles/matern52_resource_usage.txt

(`make -Otarget` keeps the remarks of concurrent compilations apart; without it the log interleaves and the table is wrong.)

The table lists VGPRs, SGPRs, scratch bytes per lane and waves per SIMD of every kernel.  It reports
  * every kernel of the first build whose numbers differ in the second (a change to existing code), and
  * every kernel that only the second build has, beside its twin: the instance of the first build whose demangled name differs in one
    template argument, 2 -> 1 (CGLB_MATERN52 -> CGLB_MATERN32).  Lower occupancy than the twin, or scratch where the twin has none, is flagged.
Exit status 1 when anything is flagged.
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m:
                cur[key] = int(m.group(1))
    return {k: v for k, v in out.items() if len(v) == len(FIELDS)}


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    short = []
    for s in res.stdout.splitlines():
        s = s.replace("(anonymous namespace)::", "")
        s = re.sub(r"^void ", "", s)
        depth, cut = 0, len(s)
        for i, ch in enumerate(s):  # drop the argument list: the first '(' outside the template brackets
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        short.append(s[:cut])
    return dict(zip(names, short))


def twin_of(name, known):
    m = re.match(r"([^<]+)<(.*)>$", name)
    if not m:
        return None
    args = [a.strip() for a in m.group(2).split(",")]
    for i, a in enumerate(args):
        if a == "2":
            cand = f"{m.group(1)}<{', '.join(args[:i] + ['1'] + args[i + 1:])}>"
            if cand in known:
                return cand
    return None


def fmt(r):
    return f"{r['vgpr']:5d} {r['sgpr']:5d} {r['scratch']:7d} {r['occ']:4d}"


def main():
    before_raw, after_raw = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(before_raw) | set(after_raw)))
    before = {names[k]: v for k, v in before_raw.items()}
    after = {names[k]: v for k, v in after_raw.items()}
    flagged = 0
    print("# VGPRs, SGPRs, scratch bytes per lane, waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    print(f"# kernels: {len(before)} before, {len(after)} after")
    print("\n## kernels of the first build: numbers before | after")
    changed = [k for k in sorted(before) if k in after and before[k] != after[k]]
    gone = [k for k in sorted(before) if k not in after]
    for k in sorted(before):  # --all lists the unchanged ones too
        if k in after and (before[k] != after[k] or "--all" in sys.argv):
            print(f"{fmt(before[k])} | {fmt(after[k])}  {'CHANGED ' if before[k] != after[k] else ''}{k}")
    print(f"\n# existing kernels with different numbers: {len(changed)}; kernels that disappeared: {len(gone)}")
    for k in gone:
        print(f"GONE {k}")
    flagged += len(changed) + len(gone)
    print("\n## new kernels: twin (before) | new instance (after)")
    lower = scratch = 0
    for k in sorted(after):
        if k in before:
            continue
        t = twin_of(k, before)
        if t is None:
            print(f"{'':26s} | {fmt(after[k])}  NO-TWIN {k}")
            flagged += 1
            continue
        note = ""
        if after[k]["occ"] < before[t]["occ"]:
            note += "LOWER-OCCUPANCY "
            lower += 1
        if after[k]["scratch"] > 0 and before[t]["scratch"] == 0:
            note += "NEW-SCRATCH "
            scratch += 1
        print(f"{fmt(before[t])} | {fmt(after[k])}  {note}{k}")
    flagged += lower + scratch
    print(f"\n# new instances below their twin's occupancy: {lower}; with scratch where the twin has none: {scratch}")
    return 1 if flagged else 0


if __name__ == "__main__":
    sys.exit(main())
