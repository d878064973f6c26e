#!/usr/bin/env python3
"""tools/isa_cmp.py PARENT_DIR THIS_DIR -- per-kernel comparison of two directories of
device assembly (tools/isa_gen.sh TREE OUT; pass OUT/prod or OUT/ab of each
tree).  Kernels are matched by mangled name.  Compared: the register, LDS,
scratch and spill figures of the kernel descriptor, and the count of every
vector-memory, LDS, MFMA, wait, barrier and sleep mnemonic.  Prints one DIFF
line per kernel that differs, `what parent->this`."""
import collections, glob, os, re, sys

CLASSES = [("vmem", re.compile(r"^(global_|buffer_|flat_|scratch_)")), ("lds", re.compile(r"^ds_")),
           ("mfma", re.compile(r"^v_mfma")), ("waitcnt", re.compile(r"^s_waitcnt")),
           ("barrier", re.compile(r"^s_barrier")), ("sleep", re.compile(r"^s_sleep"))]
META = [".vgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".sgpr_spill_count", ".vgpr_spill_count", ".sgpr_count"]


def parse(d):
    fn = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        cur = None
        meta_name = None
        pend = {}
        for line in open(path):
            s = line.strip()
            m = re.match(r"^([A-Za-z_][\w.$]*):", s)
            if m and not s.startswith(".L"):
                cur = m.group(1)
                fn.setdefault(cur, {"file": os.path.basename(path), "ins": collections.Counter(), "meta": {}})
                continue
            if s.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur and s and not s.startswith((".", ";", "//")):
                op = s.split()[0]
                for cname, rx in CLASSES:
                    if rx.match(op):
                        fn[cur]["ins"][op] += 1
            mm = re.match(r"^-?\s*(\.\w+):\s*(.*)$", s)
            if mm:
                k, v = mm.group(1), mm.group(2)
                if k == ".name":
                    if v.strip() in fn:  # a kernel's entry, not an argument's
                        meta_name = v.strip()
                        fn[meta_name]["meta"].update(pend)
                        pend = {}
                elif k in META:
                    pend[k] = v
                    # keys sort alphabetically in the YAML: .name sits in the middle
                    if meta_name in fn and k > ".name":
                        fn[meta_name]["meta"][k] = v
                        pend.pop(k)
    return fn


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    ka = {k for k, v in a.items() if v["meta"]}
    kb = {k for k, v in b.items() if v["meta"]}
    print(f"kernels: parent {len(ka)}  this {len(kb)}  only-parent {len(ka - kb)}  only-this {len(kb - ka)}")
    for k in sorted(ka - kb): print("  only parent:", a[k]["file"], k)
    for k in sorted(kb - ka): print("  only this:", b[k]["file"], k)
    byfile = collections.Counter(v["file"] for k, v in b.items() if k in kb)
    print("this kernels per file:", dict(byfile))
    byfile = collections.Counter(v["file"] for k, v in a.items() if k in ka)
    print("parent kernels per file:", dict(byfile))
    nd = 0
    for k in sorted(set(a) & set(b)):
        diffs = []
        for m in META:
            if a[k]["meta"].get(m) != b[k]["meta"].get(m): diffs.append(f"{m} {a[k]['meta'].get(m)}->{b[k]['meta'].get(m)}")
        for op in sorted(set(a[k]["ins"]) | set(b[k]["ins"])):
            if a[k]["ins"][op] != b[k]["ins"][op]: diffs.append(f"{op} {a[k]['ins'][op]}->{b[k]['ins'][op]}")
        if diffs:
            nd += 1
            print(f"DIFF {b[k]['file']} {k}: " + "; ".join(diffs))
    print("functions differing:", nd)


main()
