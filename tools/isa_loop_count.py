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

lists registers, scratch and occupancy of every kernel whose name contains KERNEL_SUBSTRING, from the compiler's notes in the file.

    python tools/isa_loop_count.py FILE.s --around KERNEL_SUBSTRING

lists what stands around that loop in the walk: the prologue (from the walk's entry to the loop) and the flush (from the barrier behind the
loop to the loop that ranks the chunk's packets).  Per part: every s_waitcnt that names vmcnt with the loads issued since the previous one,
then loads, memory atomics and vmcnt waits in program order in one line (runs counted: "8 global_load_dword | vmcnt(0)" is a batch with one
wait), and for the flush the mnemonics of its atomics; last, the atomics (LDS ones included) of the code behind the flush, the ranks and
places of the packets.  A wave waits a memory latency at a vmcnt wait that follows loads; one that follows none costs nothing new."""
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


def kernel_body(lines, key):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l)
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i] or (i > start and re.match(r"^_Z\w*:", lines[i])))
    return lines[start:end]


def parse(body):
    """the kernel's basic blocks in program order, its depth-1 loops (header label -> blocks) and the name of the walk's loop"""
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
        m = re.search(r"=>\s*This (Inner )?Loop Header: Depth=1", b["notes"])
        if m:
            name = re.match(r"^\.(LBB\w+):", b["head"]).group(1)
            loops[name] = [b]
    for b in blocks:
        for name in loops:
            if re.search(r"(Header=|Parent Loop )" + name.replace("LBB", "BB") + r"\b", b["notes"]):
                loops[name].append(b)
    # the walk: the loop that holds the LDS float atomic of the tally
    # (a sweep of rays tallies nothing: there the loop that holds GetStep's v_fract_f32 and no atomic on memory, as the event lanes' loop has)
    has = lambda n, p: any(re.match(p, i) for b in loops[n] for i in b["ins"])
    cands = ([n for n in loops if has(n, r"ds_add_f32")] or [n for n in loops if has(n, r"v_fract_f32") and not has(n, r"(global|flat|buffer)_atomic")]
             or list(loops))
    name = max(cands, key=lambda n: sum(len(b["ins"]) for b in loops[n]))
    return blocks, loops, name


LOAD = r"(global|flat|buffer)_load"
ATOMIC = r"(global|flat|buffer)_atomic"


def around(body, out=print):
    """Prologue and flush of the walk: the code on the way to its loop, and the code from the barrier behind the loop to the loop that
    ranks the chunk's packets.  Blocks are chosen by control flow (those the loop can be reached from; those reached from it) and read in
    program order.  Returns what was listed, per part: the waits as (count, loads since the previous wait), the atomics' mnemonics."""
    blocks, loops, name = parse(body)
    label = lambda b: (re.match(r"^\.(LBB\w+):", b["head"]) or [None, None])[1]
    at = {label(b): n for n, b in enumerate(blocks) if label(b)}
    succ = []
    for n, b in enumerate(blocks):
        s = [at[m.group(1)] for l in b["full"] for m in [re.match(r"s_c?branch\w*\s+\.(LBB\w+)", l)] if m and m.group(1) in at]
        if not (b["full"] and re.match(r"(s_branch|s_endpgm|s_setpc)", b["full"][-1])) and n + 1 < len(blocks):
            s.append(n + 1)
        succ.append(s)
    inloop = {n for n, b in enumerate(blocks) if any(b is c for c in loops[name])}

    def closure(seed, edges):
        seen, todo = set(), list(seed)
        while todo:
            n = todo.pop()
            for m in edges[n]:
                if m not in seen and m not in inloop:
                    seen.add(m)
                    todo.append(m)
        return seen

    pred = [[] for _ in blocks]
    for n, s in enumerate(succ):
        for m in s:
            pred[m].append(n)
    # A pass kernel holds two programs (the walk | the event workgroups), and the compiler's structured control flow lets one lead into
    # the other.  The walk's own blocks are those dominated by its entry: the first dominator of the loop's header that does not
    # dominate the kernel's other large loops.
    every = set(range(len(blocks)))
    dom = [set([0])] + [set(every) for _ in blocks[1:]]
    changed = True
    while changed:
        changed = False
        for n in range(1, len(blocks)):
            new = set.intersection(*[dom[p] for p in pred[n]]) | {n} if pred[n] else {n}
            if new != dom[n]:
                dom[n], changed = new, True
    head = at[name]
    others = [at[h] for h in loops if h != name and sum(len(b["ins"]) for b in loops[h]) > 400 and head not in dom[at[h]]]
    entry = next((d for d in sorted(dom[head], key=lambda d: len(dom[d])) if not all(d in dom[o] for o in others)), 0) if others else 0
    before = sorted(n for n in closure(inloop, pred) if entry in dom[n])
    after = sorted(n for n in closure(inloop, succ) if entry in dom[n])
    # the flush: from the first barrier behind the loop to the first loop that stores to global memory and adds no float
    stop = len(blocks)
    for h in sorted(loops, key=lambda h: at[h]):
        ins = [i for b in loops[h] for i in b["ins"]]
        if at[h] in after and any(i.startswith("global_store") for i in ins) and not any(re.search(r"atomic_(pk_)?add_f", i) for i in ins):
            stop = min(n for n, b in enumerate(blocks) if any(b is c for c in loops[h]))      # (a block of a loop may stand ahead of its header)
            break
    bar = next((n for n in after if any(i == "s_barrier" for i in blocks[n]["ins"])), None)
    flush = [n for n in after if bar is not None and bar <= n < stop]
    got = {}
    for part, sel, skip_to_barrier in (("prologue", before, False), ("flush", flush, True)):
        waits, atomics, seq, loads = [], [], [], []
        live = not skip_to_barrier
        for n in sel:
            for l in blocks[n]["full"]:
                op = l.split()[0]
                if not live:
                    live = (op == "s_barrier")
                    continue
                m = re.match(r"s_waitcnt\b.*vmcnt\((\d+)\)", l)
                if re.match(LOAD, op):
                    loads.append(op)
                    seq.append(op)
                elif re.match(ATOMIC, op):
                    atomics.append(op)
                    seq.append(op)
                elif m:
                    waits.append((int(m.group(1)), loads))
                    out("%-8s s_waitcnt vmcnt(%s) in block %s after the loads: %s" % (part, m.group(1), label(blocks[n]) or "(fall-through)",
                                                                                       ", ".join(runs(loads)) or "-"))
                    loads = []
                    seq.append("vmcnt(%s)" % m.group(1))
        out("%-8s order of loads, atomics and vmcnt waits: %s" % (part, " | ".join(runs(seq)) or "-"))
        if part == "flush":
            out("flush    atomics: %s" % (", ".join(runs(sorted(atomics))) or "-"))
        got[part] = {"waits": waits, "atomics": atomics, "order": seq}
    # behind the flush (the ranks and places of the chunk's packets): the atomics, LDS ones included
    rank = [l.split()[0] for n in after if n >= stop for l in blocks[n]["full"] if re.match(ATOMIC + r"|ds_(add|cmpst)", l)]
    out("ranks    atomics: %s" % (", ".join(runs(sorted(rank))) or "-"))
    got["ranks"] = {"atomics": rank}
    return got


def runs(ops):
    """['a', 'a', 'b'] -> ['2 a', 'b']"""
    res = []
    for o in ops:
        if res and res[-1][1] == o:
            res[-1][0] += 1
        else:
            res.append([1, o])
    return [("%d %s" % (n, o)) if n > 1 else o for n, o in res]


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    if key == "--resources":
        return resources(lines, sys.argv[3])
    if key == "--around":
        around(kernel_body(lines, sys.argv[3]))
        return
    blocks, loops, name = parse(kernel_body(lines, key))
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
