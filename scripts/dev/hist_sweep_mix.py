"""Basic blocks of one kernel in a compiler assembly file, with instruction counts by class (development; no GPU).
    python scripts/dev/hist_sweep_mix.py hist_planned.s '_ZN4pisa19hist_planned_kernelE' [first_block last_block]
hist_planned.s: hist_planned.hip compiled with the Makefile's flags plus `-S --cuda-device-only`.  Without a block range: one line per
basic block (label, loop depth, counts, where it branches to) -- enough to follow the path a wavefront takes through the
sweep; with a range: the totals over those blocks (the blocks of the all-fast path of one sweep are contiguous)."""
import collections, re, sys

lines = open(sys.argv[1]).read().splitlines()
sym = sys.argv[2]
start = next(i for i, l in enumerate(lines) if l.startswith(sym) and l.split(";")[0].rstrip().endswith(":"))
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))


def cls(op):
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "valu"


blocks, cur = [], None
for l in lines[start + 1:end]:
    m = re.match(r"^(\.LBB[0-9_]+):", l)
    if m or cur is None:
        cur = {"label": m.group(1) if m else "entry", "depth": "", "n": collections.Counter(), "to": [], "ops": collections.Counter()}
        blocks.append(cur)
        if m:
            continue
    d = re.search(r"Depth=(\d+)", l)
    if d and not cur["depth"]:
        cur["depth"] = d.group(1)
    m = re.match(r"^\s+([a-z][a-z0-9_]+)\s*(.*?)\s*(;.*)?$", l)
    if not m or l.lstrip().startswith("."):
        continue
    op = m.group(1)
    cur["n"][cls(op)] += 1
    cur["ops"][op] += 1
    if cls(op) == "branch":   # a block ends at its branch: what follows is LABEL+k
        cur["to"].append(op.replace("s_cbranch_", "").replace("s_branch", "always") + ">" + m.group(2).strip())
        base, _, k = cur["label"].partition("+")
        cur = {"label": "%s+%d" % (base, int(k or 0) + 1), "depth": cur["depth"], "n": collections.Counter(), "to": [], "ops": collections.Counter()}
        blocks.append(cur)

order = ["valu", "salu", "branch", "lds", "vmem", "smem", "wait"]
if len(sys.argv) > 4:
    lo = next(i for i, b in enumerate(blocks) if b["label"] == sys.argv[3])
    hi = next(i for i, b in enumerate(blocks) if b["label"] == sys.argv[4])
    tot, ops = collections.Counter(), collections.Counter()
    for b in blocks[lo:hi + 1]:
        tot.update(b["n"])
        ops.update(b["ops"])
    print("blocks %s .. %s (%d):" % (sys.argv[3], sys.argv[4], hi - lo + 1), " ".join("%s=%d" % (k, tot[k]) for k in order),
          "total=%d" % sum(tot.values()))
    print("  " + " ".join("%s:%d" % kv for kv in ops.most_common()))
else:
    for b in blocks:
        if sum(b["n"].values()) == 0:
            continue
        print("%-12s d=%-2s %s  -> %s" % (b["label"], b["depth"], " ".join("%s=%-3d" % (k, b["n"][k]) for k in order), ", ".join(b["to"])))
