#!/usr/bin/env python3
"""Per-kernel comparison of two `hipcc --cuda-device-only -S` listings of one source file (a refactor's parent against its new build):

    tools/stream_diff.py parent.s new.s

For every kernel: instruction count, VGPR, SGPR, LDS, scratch, spills and v_mfma count (from the amdhsa.kernels metadata and the
stream), and whether the ordered subsequence of matrix, memory and synchronisation opcodes (v_mfma*, buffer_*, global_*, ds_*,
s_waitcnt with its counters, s_barrier, s_setprio) is the same.  Exit status 1 if a kernel breaks the rule a hand-scheduled kernel is
held to: equal instruction, MFMA and LDS figures, no more VGPRs, scratch or spills, the same ordered subsequence."""
import re
import subprocess
import sys

KEEP = ("v_mfma", "buffer_", "global_", "ds_", "s_waitcnt", "s_barrier", "s_setprio")


def kernels(path):
    text = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        get = lambda key: (re.search(r"\n    \." + key + r":\s*(\S+)", blk) or [None, "0"])[1]
        meta[get("name")] = {k: int(get(k)) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size",
                                                       "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        if m.group(1) not in meta:
            continue
        ins = [l.split(";")[0].split() for l in m.group(2).splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        ins = [i for i in ins if i]
        seq = [" ".join(i) if i[0] == "s_waitcnt" else i[0] for i in ins if i[0].startswith(KEEP)]
        out[m.group(1)] = dict(meta[m.group(1)], n=len(ins), mfma=sum(i[0].startswith("v_mfma") for i in ins), seq=seq,
                               ops=sorted(i[0] for i in ins))
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    names = subprocess.run(["c++filt"], input="\n".join(a), capture_output=True, text=True).stdout.split("\n")
    bad = 0
    pair = lambda x, y: f"{x} = {y}" if x == y else f"{x} -> {y}"
    print(f"{'kernel':66s} {'stream':10s} {'instructions':14s} {'VGPR':11s} {'SGPR':10s} {'LDS':9s} scratch  spills  MFMA       opcodes")
    for sym, name in zip(a, names):
        name = re.sub(r"^void \(anonymous namespace\)::|\(.*$", "", name)
        p, n = a[sym], b.get(sym)
        if n is None:
            print(f"{name:66s} MISSING in the new listing")
            bad += 1
            continue
        same_seq = p["seq"] == n["seq"]
        ok = (same_seq and p["n"] == n["n"] and p["mfma"] == n["mfma"] and p["group_segment_fixed_size"] == n["group_segment_fixed_size"]
              and all(n[k] <= p[k] for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")))
        bad += not ok
        stream = "identical" if same_seq and p["ops"] == n["ops"] else ("same-seq" if same_seq else "CHANGED")
        print(f"{name:66s} {stream:10s} {pair(p['n'], n['n']):14s} {pair(p['vgpr_count'], n['vgpr_count']):11s} "
              f"{pair(p['sgpr_count'], n['sgpr_count']):10s} {pair(p['group_segment_fixed_size'], n['group_segment_fixed_size']):9s} "
              f"{pair(p['private_segment_fixed_size'], n['private_segment_fixed_size']):8s} "
              f"{pair(p['vgpr_spill_count'], n['vgpr_spill_count']):7s} {pair(p['mfma'], n['mfma']):10s} "
              f"{'same multiset' if p['ops'] == n['ops'] else 'multiset differs'}{'' if ok else '   <-- BREAKS THE RULE'}")
    extra = [s for s in b if s not in a]
    if extra:
        print("only in the new listing:", extra)
        bad += len(extra)
    print(f"{len(a)} kernels compared, {bad} break the rule")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
