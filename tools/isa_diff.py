"""Per-kernel comparison of two hipcc assembly files (CPU only; companion of isa_histogram.py).

    hipcc <the file's Makefile flags> --cuda-device-only -S -o old.s old/lg_ffn.hip
    hipcc <the same flags>            --cuda-device-only -S -o new.s new/lg_ffn.hip
    python tools/isa_diff.py old.s new.s [--map names.txt] [--show N]

Splits both files per kernel symbol, strips `;` comments, drops the function index from
`.LBB<n>_<m>` labels (removing a kernel renumbers every later function) and compares, for
every symbol present in both files, the instruction text and the `.amdhsa_kernel`
descriptor block (registers, LDS, scratch).  Prints the removed, added and differing
symbols; exit status 1 if any symbol differs or was added.

--map FILE: lines `old new` (or --rename OLD=NEW, repeatable) for kernels whose mangled name
changed, e.g. by a dropped template parameter: every occurrence of `old` in the old file
(a whole symbol, or the part of it that changed) is rewritten to `new` first, so the old
kernel is compared with the new one under the new name."""
import argparse
import difflib
import re
import sys


def parse(path, rename):
    """{symbol: (instruction lines, descriptor lines)} of one assembly file."""
    text = open(path).read()
    applied = 0
    for old, new in rename.items():
        applied += old in text
        text = text.replace(old, new)
    body, desc = {}, {}
    cur = dcur = None
    for ln in text.split("\n"):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            dcur = m.group(1)
            desc[dcur] = []
            continue
        if dcur is not None:
            if ".end_amdhsa_kernel" in ln:
                dcur = None
            else:
                desc[dcur].append(" ".join(ln.split(";")[0].split()))
            continue
        if cur is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
            if m and not m.group(1).startswith(".L"):
                cur = m.group(1)
                body[cur] = []
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        t = " ".join(ln.split(";")[0].split())
        if t:
            body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    # a symbol with a body but no descriptor is a device function, not a kernel
    return {k: (body[k], desc[k]) for k in body if k in desc}, applied


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", help="file of `old_symbol new_symbol` lines")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--show", type=int, default=0, help="print the first N diff lines of each differing symbol")
    a = ap.parse_args()
    rename = {}
    if a.map:
        for ln in open(a.map):
            f = ln.split("#")[0].split()
            if len(f) == 2:
                rename[f[0]] = f[1]
    for r in a.rename:
        old, new = r.split("=", 1)
        rename[old] = new
    (old, nren), (new, _) = parse(a.old, rename), parse(a.new, {})
    common = [k for k in old if k in new]
    removed = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    differing = [k for k in common if old[k] != new[k]]
    print(f"{a.old} -> {a.new}: old {len(old)} kernels, new {len(new)}, common {len(common)}, "
          f"renames applied {nren}, differing {len(differing)}, added {len(added)}, removed {len(removed)}")
    for k in differing:
        what = [w for w, i in (("text", 0), ("descriptor", 1)) if old[k][i] != new[k][i]]
        print(f"  differs ({' + '.join(what)}): {k}")
        if a.show:
            d = difflib.unified_diff(old[k][0] + old[k][1], new[k][0] + new[k][1], "old", "new", lineterm="", n=1)
            for ln in list(d)[:a.show]:
                print("      " + ln)
    for k in added:
        print(f"  added: {k}")
    for k in removed:
        print(f"  removed: {k}")
    return 1 if differing or added else 0


if __name__ == "__main__":
    sys.exit(main())
