"""What does every kernel of a source file take: registers, scratch, occupancy, spills, static LDS?  Compiles the given
sources of a csrc directory for the device alone with the library's own flags (cellregmap_amd/build.py) plus
-Rpass-analysis=kernel-resource-usage and prints one row per demangled kernel from the compiler's remarks -- nothing is
run and no assembly is parsed.  With --against, the same sources of another csrc directory (e.g. the parent commit in a
`git worktree`; a source missing there is skipped) are compiled too and the rows that differ are printed behind the table,
kernels of either side without a partner included.  --asm keeps the device assembly of every source under a directory,
for a diff by other means.
    python tools/diag/kernel_resources.py <csrc dir> <file.hip>... [--against <other csrc dir>] [--asm <dir>]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# remark label -> column
FIELDS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "LDS"))
COLUMNS = tuple(col for _, col in FIELDS)
REMARK = re.compile(r"remark: (?:.*?:\d+:\d+: )?\s*([A-Za-z][A-Za-z \[\]/]*?): (\S+)")


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()

    def short(s):   # without the return type, the namespaces and the parameter list: gram_ext_kernel<12, 2>
        s = re.sub(r"^void ", "", s.replace("(anonymous namespace)::", "").replace("crm::", ""))
        depth = 0
        for i, ch in enumerate(s):
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                return s[:i]
        return s

    return {n: short(d) for n, d in zip(names, out)}


def resources(csrc, source, asm_dir=None):
    """{kernel: {column: int}} of one source file, from the remarks of a device-only compilation."""
    from cellregmap_amd import build

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(asm_dir or tmp, source.replace(".hip", ".s"))
        cmd = [build.HIPCC, *build.CXXFLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
               os.path.join(csrc, source), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (source, r.stderr))
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        label, value = m.group(1).strip(), m.group(2)
        if label == "Function Name":
            cur = rows.setdefault(value, {})
        elif cur is not None:
            for name, col in FIELDS:
                if label == name:
                    cur[col] = int(value)
    names = demangle(list(rows))
    return {names[k]: v for k, v in rows.items() if v}


def table(csrc, sources, asm_dir=None):
    if asm_dir:
        os.makedirs(asm_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=4) as ex:
        parts = list(ex.map(lambda s: resources(csrc, s, asm_dir), sources))
    return {kernel: row for part in parts for kernel, row in part.items()}


def fmt(kernel, row, width):
    return kernel.ljust(width) + " " + " ".join("%s %4s" % (c, row.get(c, "-")) for c in COLUMNS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csrc")
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--against", help="another csrc directory: print the rows that differ from it")
    ap.add_argument("--asm", help="keep the device assembly here (<dir>/this, <dir>/against)")
    args = ap.parse_args()
    here = table(args.csrc, args.sources, args.asm and os.path.join(args.asm, "this"))
    width = max(map(len, here), default=0)
    for kernel in sorted(here):
        print(fmt(kernel, here[kernel], width))
    if not args.against:
        return 0
    there = table(args.against, [s for s in args.sources if os.path.exists(os.path.join(args.against, s))],
                  args.asm and os.path.join(args.asm, "against"))
    moved = [k for k in sorted(set(here) | set(there)) if here.get(k) != there.get(k)]
    print("\n%d kernels here, %d there, %d rows differ" % (len(here), len(there), len(moved)))
    for kernel in moved:
        for tag, side in (("there", there), ("here ", here)):
            print(tag + " " + (fmt(kernel, side[kernel], width) if kernel in side else kernel.ljust(width) + " (absent)"))
    lost = [k for k in moved if k in here and k in there and
            (here[k]["occ"] < there[k]["occ"] or here[k]["scratch"] > there[k]["scratch"] or here[k]["vspill"] > there[k]["vspill"])]
    for kernel in lost:
        print("LOST: %s has lower occupancy, more scratch or more VGPR spills here" % kernel)
    return 1 if lost else 0


if __name__ == "__main__":
    sys.exit(main())
