#!/usr/bin/env python3
"""Static instruction mix of the main loop of a kernel in a --save-temps .s file (development aid).

    python tools/isa_loop_count.py FILE.s KERNEL_SUBSTRING

Finds the kernel whose (mangled) name contains KERNEL_SUBSTRING, takes the depth-1 loop that holds the tally's ds_add_f32 and counts VALU / SALU /
LDS / VMEM instructions of the basic blocks that belong to it, split at the first v_fract_f32 (swap arm | step arm).  Per arm it then lists
every s_waitcnt that names vmcnt, with the global loads and stores issued before it in the same arm (in program order): a wait that follows
loads of its own arm with a count below the accesses issued since waits for memory the arm asked for itself.  For the step arm it lists
every s_waitcnt that names lgkmcnt with the LDS operations issued before it in the arm -- the loop issues no scalar-memory or FLAT operation,
so lgkmcnt counts LDS operations only, and those retire in order: a wait with a count below the operations issued since waits for the
oldest of them -- and says how many ds_add_f32 stand between the aim read (the first ds_read_b32 of the arm) and the last wait of the
descent loop (the inner loop that reads LDS): none, when the tally is issued after the landing.

    python tools/isa_loop_count.py FILE.s --resources KERNEL_SUBSTRING

lists registers, scratch and occupancy of every kernel whose name contains KERNEL_SUBSTRING, from the compiler's notes in the file."""
import re
import sys


def resources(lines, key):
    name = None
    got = {}
    for l in lines:
        m = re.match(r"^(_Z\w*):", l)
        if m:
            name, got = m.group(1), {}
        m = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", l)
        if m and name:
            got[m.group(1)] = m.group(2)
            if m.group(1) == "Occupancy" and key in name:
                print("%-60s VGPRs %3s  AGPRs %s  scratch %3s B  occupancy %s waves/SIMD" % (
                    re.sub(r"Ev7SocGrid.*", "E", name), got.get("NumVgprs"), got.get("NumAgprs"), got.get("ScratchSize"), got["Occupancy"]))


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    if key == "--resources":
        return resources(lines, sys.argv[3])
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l)
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i] or (i > start and re.match(r"^_Z\w*:", lines[i])))
    body = lines[start:end]
    # blocks: label line or '; %bb.N:' comment starts a block; membership from the 'in Loop: Header=X' / 'Parent Loop X' / 'This Loop Header' notes
    blocks, cur = [], None
    for l in body:
        if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", l):
            cur = {"head": l, "notes": l, "ins": [], "full": [], "inner": False}
            blocks.append(cur)
        elif cur is not None:
            if l.strip().startswith(";"):
                cur["notes"] += " " + l
                cur["inner"] = cur["inner"] or bool(re.search(r"Depth=2", l))
            elif l.strip() and not l.strip().startswith("."):
                cur["ins"].append(l.strip().split()[0])
                cur["full"].append(l.strip())
    loops = {}
    for b in blocks:
        m = re.search(r"=>\s*This Loop Header: Depth=1", b["notes"])
        if m:
            name = re.match(r"^\.(LBB\w+):", b["head"]).group(1)
            loops[name] = [b]
    for b in blocks:
        for name in loops:
            if re.search(r"(Header=|Parent Loop )" + name.replace("LBB", "BB") + r"\b", b["notes"]):
                loops[name].append(b)
    # the walk: the loop that holds the LDS float atomic of the tally
    cands = [n for n in loops if any(i.startswith("ds_add_f32") for b in loops[n] for i in b["ins"])] or list(loops)
    name = max(cands, key=lambda n: sum(len(b["ins"]) for b in loops[n]))
    order = [b for b in blocks if b in loops[name]]
    seen_fract = False
    part = {"swap": [], "step": []}
    full = {"swap": [], "step": []}
    step_inner = []                                          # per instruction of the step arm: does it stand in an inner loop that reads LDS
    for b in order:
        if any(i.startswith("v_fract") for i in b["ins"]) or any(i.startswith("v_trunc") for i in b["ins"]):
            seen_fract = True
        part["step" if seen_fract else "swap"] += b["ins"]
        full["step" if seen_fract else "swap"] += b["full"]
        if seen_fract:
            step_inner += [b["inner"] and any(i.startswith("ds_read") for i in b["ins"])] * len(b["full"])
    for k, ins in part.items():
        c = lambda p: sum(1 for i in ins if re.match(p, i))
        print("%-5s VALU %4d  SALU %4d  LDS %3d  VMEM %3d   (v_mov %d, v_cndmask %d, v_cmp %d)" % (
            k, c(r"v_"), c(r"s_"), c(r"ds_"), c(r"(global|flat|buffer)_"), c(r"v_mov"), c(r"v_cndmask"), c(r"v_cmp")))
    for k, ins in full.items():
        print("%-5s ds_add_rtn (the reservation of the swap arm: one per wave when the compiler aggregates the lanes' additions): %d" % (
            k, sum(1 for l in ins if l.startswith("ds_add_rtn"))))
        loads = stores = 0
        for n, l in enumerate(ins):
            if re.match(r"(global|flat|buffer)_load", l):
                loads += 1
            elif re.match(r"(global|flat|buffer)_(store|atomic)", l):
                stores += 1
            m = re.match(r"s_waitcnt\b.*vmcnt\((\d+)\)", l)
            if m:
                print("%-5s instruction %3d: s_waitcnt vmcnt(%s) after %d global loads and %d global stores of this arm" % (k, n, m.group(1), loads, stores))
    # the step arm's waits for LDS, in program order
    ins, lds, aim, last = full["step"], [], None, None
    for n, l in enumerate(ins):
        if l.startswith("ds_"):
            lds.append((n, l.split()[0]))
            if aim is None and l.startswith("ds_read_b32"):
                aim = n
        m = re.match(r"s_waitcnt\b.*lgkmcnt\((\d+)\)", l)
        if m:
            print("step  instruction %3d: s_waitcnt lgkmcnt(%s)%s after the LDS operations %s" % (
                n, m.group(1), " in the descent loop" if step_inner[n] else "", ", ".join("%s (%d)" % (o, i) for i, o in lds) or "-"))
            if step_inner[n]:
                last = n
    if aim is not None and last is not None:
        print("step  ds_add_f32 between the aim read (instruction %d) and the last wait of the descent loop (instruction %d): %d" % (
            aim, last, sum(1 for i, o in lds if o.startswith("ds_add_f32") and aim < i < last)))


if __name__ == "__main__":
    main()
