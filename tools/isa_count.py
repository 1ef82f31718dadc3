#!/usr/bin/env python3
"""Static instruction mix of the main loop of device kernels, from the ISA hipcc emits (round 5: the evidence that the Winograd /
stride-2 kernels were bound by their own instruction count -- DESIGN.md section 4.1), and (round 7) a report of the vector-memory
waits of their item loops.

    hipcc --offload-arch=gfx950 <Makefile FLAGS> --save-temps -c gsa_kernels.hip   (writes *-hip-amdgcn-amd-amdhsa-gfx950.s)
    python tools/isa_count.py <file.s> [substring of the demangled kernel name ...]
    python tools/isa_count.py --waits <file.s> [substring ...]
    python tools/isa_count.py --dma-waits <file.s> [substring ...]

For every matching kernel: the instructions between the head of its LARGEST loop and that loop's back edge, by class.  The count is
static -- both the border and the interior staging path are in it, and an epilogue that runs once per tile is counted once per item --
so it overstates a streamed-weight kernel's per-item work; it compares like with like between two kernels of the same structure.

--waits: for every matching kernel and every innermost ITEM loop (a loop that holds MFMAs and a barrier and no smaller such loop):
  * per iteration, on the path through the loop body that issues the most of them: the vector-memory loads, LDS-DMA pieces
    (global_load_lds), stores and atomics -- the numbers a hand-written counted wait assumes;
  * every `s_waitcnt vmcnt(N)` of the loop with what was issued since the previous barrier on the longest path that reaches it (the
    state at the back edge carried round to the loop head) and between the two barriers before that, and whether a path from a
    barrier reaches it without an MFMA ("top": the wait sits in front of the item's staging).
vmcnt counts loads, LDS-DMA pieces, stores and atomics alike on this architecture and retires only loads in order: a wait at the top
of an iteration with N below the stores and atomics the previous iteration's epilogue left in flight makes the item wait for their
acknowledgement.  The walk takes inner loops once.
--dma-waits: the same report for the innermost loops that hold LDS-DMA pieces, whatever else they hold (post_dma: each wave walks
its rows behind counted waits of its own, without MFMAs or barriers)."""
import collections
import re
import subprocess
import sys


def cat(op):
    for prefix, name in (("v_mfma", "mfma"), ("v_pk_", "valu_pk"), ("v_accvgpr", "accvgpr"), ("v_", "valu"), ("ds_read", "lds_read"),
                         ("ds_write", "lds_write"), ("ds_", "lds_other"), ("global_load_lds", "lds_dma"), ("global_load", "vmem_load"),
                         ("buffer_load", "vmem_load"), ("global_store", "vmem_store"), ("global_atomic", "atomic"), ("scratch_", "scratch"),
                         ("s_waitcnt", "s_waitcnt"), ("s_barrier", "s_barrier"), ("s_nop", "s_nop"), ("s_load", "smem"), ("s_buffer", "smem"), ("s_", "salu")):
        if op.startswith(prefix):
            return name
    return "other"


VM_KINDS = ("vmem_load", "lds_dma", "vmem_store", "atomic")      # what the vector-memory counter counts


def kernels(src, filters=()):
    """(mangled name, demangled name, body lines) of every kernel of an assembly file whose demangled name holds one of `filters`."""
    names = re.findall(r"^(_Z\w+):\s*; @", src, re.M)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    for name, d in zip(names, dem):
        if filters and not any(f in d for f in filters):
            continue
        m = re.search(r"^" + re.escape(name) + r":.*?^\s*s_endpgm", src, re.S | re.M)
        if m:
            yield name, d, m.group(0).split("\n")


def short_name(d):
    return d.replace("void gsa::", "").replace("(gsa::ConvParams)", "").replace("(gsa::PostParams)", "")


def loops_of(body):
    """(head, back edge) line indices of every loop: a branch to a label above it."""
    labels = {mm.group(1): i for i, l in enumerate(body) for mm in [re.match(r"^(\.LBB\d+_\d+):", l)] if mm}
    loops = []
    for i, l in enumerate(body):
        mm = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", l)
        if mm:
            t = mm.group(1) or mm.group(2)
            if t in labels and labels[t] < i:
                loops.append((labels[t], i))
    return labels, loops


def opcode(line):
    l = line.strip()
    if not l or l[0] in ";." or l.endswith(":"):
        return None
    return l.split()[0]


def count_main_loop(body):
    _, loops = loops_of(body)
    if not loops:
        return None
    a, b = max(loops, key=lambda x: x[1] - x[0])
    c = collections.Counter()
    for l in body[a:b + 1]:
        op = opcode(l)
        if op:
            c[cat(op)] += 1
    return c


BRANCH = re.compile(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)")


def successors(body, labels):
    """Line -> lines control can go to next (the whole kernel; blocks need not be laid out in execution order)."""
    succ = []
    for i, l in enumerate(body):
        out = []
        mm = BRANCH.search(l)
        if mm:
            t = labels.get(mm.group(1) or mm.group(2))
            if t is not None:
                out.append(t)
        if not (mm and mm.group(2)) and opcode(l) != "s_endpgm" and i + 1 < len(body):
            out.append(i + 1)      # a conditional branch or no branch: falls through
        succ.append(out)
    return succ


def depth_first(root, edges):
    """(lines reachable from root in topological order of the graph without its cycle-closing edges, those edges)."""
    state, topo, stack, closing = {root: 1}, [], [(root, iter(edges[root]))], set()
    while stack:
        i, it = stack[-1]
        for t in it:
            if state.get(t) == 1:
                closing.add((i, t))
            elif t not in state:
                state[t] = 1
                stack.append((t, iter(edges[t])))
                break
        else:
            state[i] = 2
            topo.append(i)
            stack.pop()
    topo.reverse()
    return topo, closing


def reach(start, edges, stop=None):
    seen, todo = set(start), list(start)
    while todo:
        i = todo.pop()
        for t in edges[i]:
            if t != stop and t not in seen:
                seen.add(t)
                todo.append(t)
    return seen


def item_loops(body, dma_loops=False):
    """(head, member lines, latches) of the innermost loops that hold both MFMAs and a barrier -- dma_loops: that hold LDS-DMA pieces,
    for the kernels whose waves walk rows on their own (post_dma: no MFMA, no barrier).  A loop is the lines that can be reached from
    its head and can reach a branch back to it (its latches) without passing the head."""
    labels, _ = loops_of(body)
    succ = successors(body, labels)
    pred = [[] for _ in body]
    for i, out in enumerate(succ):
        for t in out:
            pred[t].append(i)
    # the edges that close a cycle, by a depth-first walk from the kernel's entry: where a branch points in the TEXT says nothing (the
    # compiler lays blocks out above their predecessors and latches above their heads)
    back = depth_first(0, succ)[1]
    cand = []
    for a in sorted({t for _, t in back}):
        latches = [i for i, t in back if t == a]
        members = reach([a], succ, stop=a) & reach(latches, pred, stop=a) | {a}
        ops = [opcode(body[i]) for i in members]
        if (any(o and o.startswith("global_load_lds") for o in ops) if dma_loops else
                any(o and o.startswith("v_mfma") for o in ops) and any(o == "s_barrier" for o in ops)):
            cand.append((a, members, [i for i in latches if i in members]))
    return labels, succ, [c for c in cand if not any(o[1] < c[1] for o in cand)]


def walk_loop(body, succ, a, members, latches):
    """Longest-path walk over one iteration of a loop.  Returns (per-iteration maxima, waits)."""
    zero = (0, 0, 0, 0)
    # inner loops are taken once: the edges that close a cycle (found by a depth-first walk from the head) are left out, and the rest
    # is walked in topological order, whatever order the compiler laid the blocks out in
    edges = {i: [t for t in succ[i] if t != a and t in members] for i in members}
    topo, closing = depth_first(a, edges)
    order = sorted(members)

    def run(head_state, head_clean):
        # since[i]: the (loads, dma, stores, atomics) with the largest total issued since the last barrier on a path from the head to i,
        # behind what had been issued between the two barriers before that; whole[i]: the same without the reset (per-iteration
        # maximum); clean[i]: some path from a barrier reaches i without an MFMA (the loop head is whatever block the compiler rotated
        # to the top: an iteration of the source begins behind its closing barrier)
        since, whole, clean, out = {a: head_state}, {a: zero}, {a: head_clean}, {}
        for i in topo:
            s, w, c = since[i], whole[i], clean[i]
            op = opcode(body[i])
            if op:
                k = cat(op)
                if k in VM_KINDS:
                    j = VM_KINDS.index(k)
                    s = s[:4] + tuple(v + (1 if n == j else 0) for n, v in enumerate(s[4:]))
                    w = tuple(v + (1 if n == j else 0) for n, v in enumerate(w))
                elif k == "s_barrier":
                    s, c = s[4:] + zero, True
                elif k == "mfma":
                    c = False
            out[i] = (s, w, c)
            for t in edges[i]:
                if (i, t) in closing:
                    continue
                if t not in since or sum(s[4:]) > sum(since[t][4:]):
                    since[t] = s
                if t not in whole or sum(w) > sum(whole[t]):
                    whole[t] = w
                clean[t] = clean.get(t, False) or c
        end_since = max((out[i][0] for i in latches if i in out), key=sum, default=zero + zero)
        end_whole = max((out[i][1] for i in latches if i in out), key=sum, default=zero)
        return since, clean, end_since, end_whole, any(out[i][2] for i in latches if i in out)

    _, _, end_since, _, end_clean = run(zero + zero, False)
    since, clean, _, end_whole, _ = run(end_since, end_clean)      # the back edge's state carried round to the head
    waits = []
    for i in order:
        if i in since and opcode(body[i]) == "s_waitcnt":
            mm = re.search(r"vmcnt\((\d+)\)", body[i])
            if mm:
                waits.append({"n": int(mm.group(1)), "line": i, "top": clean[i],
                              **dict(zip(("prev_loads", "prev_dma", "prev_stores", "prev_atomics", "loads", "dma", "stores", "atomics"), since[i]))})
    per_iter = dict(zip(("loads", "dma", "stores", "atomics"), end_whole))
    return per_iter, waits


def static_counts(body, members):
    """Every global_load_lds / global_load / global_store / atomic of the loop text, whichever path holds it."""
    c = collections.Counter()
    for i in members:
        op = opcode(body[i])
        if op and cat(op) in VM_KINDS:
            c[cat(op)] += 1
    return {"loads": c["vmem_load"], "dma": c["lds_dma"], "stores": c["vmem_store"], "atomics": c["atomic"]}


def waits_report(src, filters=(), dma_loops=False):
    """[{name, loops: [{head, per_iter, static, waits}]}] for the kernels of an assembly text (see the module docstring)."""
    out = []
    for name, d, body in kernels(src, filters):
        labels, succ, loops = item_loops(body, dma_loops)
        lps = []
        for a, members, latches in loops:
            per_iter, waits = walk_loop(body, succ, a, members, latches)
            lps.append({"head": body[a].split(":")[0], "per_iter": per_iter, "static": static_counts(body, members), "waits": waits})
        if lps:
            out.append({"name": short_name(d), "mangled": name, "loops": lps})
    return out


def false_store_waits(loop):
    """The waits at the top of an iteration (no MFMA since a barrier on some path) that make the item wait for the previous item's
    output: the count, less what the iteration itself has issued since the barrier, is below the stores and atomics an iteration can
    leave in flight.  A wait whose count is below what has been issued since the barrier waits for one of THOSE operations (the AdaIN
    coefficients on a sample change, read where they are used) and is no such wait, whatever else it drains on that rare path."""
    in_flight = loop["per_iter"]["stores"] + loop["per_iter"]["atomics"]
    out = []
    for w in loop["waits"]:
        issued = w["loads"] + w["dma"] + w["stores"] + w["atomics"]
        if w["top"] and issued <= w["n"] < issued + in_flight:
            out.append(w)
    return out


def print_waits(src, filters, dma_loops=False):
    for k in waits_report(src, filters, dma_loops):
        print(k["name"])
        for lp in k["loops"]:
            p, s = lp["per_iter"], lp["static"]
            print("  loop %s  per iteration (longest path): load %d  dma %d  store %d  atomic %d   in the loop text: load %d  dma %d  store %d  atomic %d"
                  % (lp["head"], p["loads"], p["dma"], p["stores"], p["atomics"], s["loads"], s["dma"], s["stores"], s["atomics"]))
            bad = {w["line"] for w in false_store_waits(lp)}
            for w in lp["waits"]:
                print("    vmcnt(%d)%s  since the barrier: load %d  dma %d  store %d  atomic %d   before it: load %d  dma %d  store %d  atomic %d%s"
                      % (w["n"], " top" if w["top"] else "    ", w["loads"], w["dma"], w["stores"], w["atomics"],
                         w["prev_loads"], w["prev_dma"], w["prev_stores"], w["prev_atomics"],
                         "   <-- waits for the previous item's stores" if w["line"] in bad else ""))


def main():
    args = sys.argv[1:]
    waits, dma_loops = "--waits" in args or "--dma-waits" in args, "--dma-waits" in args
    args = [x for x in args if x not in ("--waits", "--dma-waits")]
    src = open(args[0]).read()
    filters = args[1:]
    if waits:
        print_waits(src, filters, dma_loops)
        return
    for name, d, body in kernels(src, filters):
        c = count_main_loop(body)
        if c is None:
            continue
        order = ["mfma", "valu", "valu_pk", "salu", "lds_read", "lds_write", "lds_dma", "vmem_load", "vmem_store", "s_waitcnt", "s_nop", "scratch"]
        print("%-62s %s  total %d" % (short_name(d)[:62], " ".join("%s %d" % (k, c[k]) for k in order if c[k]), sum(c.values())))


if __name__ == "__main__":
    main()
