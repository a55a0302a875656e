"""Hand check for k_sor_rbp (no GPU): instruction counts between consecutive s_barrier in the gfx950 assembly of one kernel.
    hipcc <build.py's CFLAGS> --cuda-device-only -S -o sor5.s csrc/pdeip_sor5.hip
    python tools/rbp_isa_count.py sor5.s [MODEL [FIRST]]          (ModelElin4, 1)
Prints the kernel's resources and, for every stretch of straight-line code between two barriers (no branch inside: the steps
of a steady-state march are such stretches), VALU / SALU / LDS / global-store counts, grouped by equal counts."""
import collections, re, sys
path = sys.argv[1]
model = sys.argv[2] if len(sys.argv) > 2 else "ModelElin4"
first = sys.argv[3] if len(sys.argv) > 3 else "1"
want = re.compile(r"^_ZN5pdeip9k_sor_rbpINS_\d+%sELi4ELb%sE[^:]*:" % (model, first))
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if want.match(l) and not l.startswith("\t"))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
name = lines[start].rstrip(":")
for l in lines[end:end + 80]:
    m = re.match(r"\s*; (NumVgprs|NumSgprs|ScratchSize|codeLenInByte|Occupancy)\b.*", l)
    if m: print(l.strip("; \t"))
seg, segs, branchy = collections.Counter(), [], False
for l in lines[start + 1:end]:
    op = l.split()[0] if l.startswith("\t") and l.split() else ""
    if not op or op.startswith((".", ";")):
        if l and not l.startswith(("\t", ";")) and l.rstrip().endswith(":"): branchy = True  # a label: a branch target
        continue
    if op == "s_barrier":
        segs.append((branchy, seg))
        seg, branchy = collections.Counter(), False
        continue
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")): branchy = True
    elif op.startswith("v_"): seg["valu"] += 1
    elif op.startswith("ds_"): seg["lds"] += 1
    elif op.startswith(("global_store", "flat_store")): seg["gst"] += 1
    elif op.startswith(("global_load", "buffer_load")): seg["gld"] += 1
    elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop")): seg["salu"] += 1
print("%d barriers; straight-line stretches between two of them:" % len(segs))
groups = collections.Counter((s["valu"], s["salu"], s["lds"], s["gst"], s["gld"]) for b, s in segs[1:] if not b)
for (v, sa, ld, gs, gl), n in sorted(groups.items()):
    print("  %2d x   VALU %3d   SALU %3d   LDS %2d   global stores %d   DMA %d" % (n, v, sa, ld, gs, gl))
print("stretches with a branch or a label inside: %d" % sum(1 for b, s in segs[1:] if b))
