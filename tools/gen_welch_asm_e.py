#!/usr/bin/env python3
"""Generator (and CPU emulator) of `mdsp_welch_w64e_asm` (Welch variant 45): the folded-twiddle Welch kernel of tools/gen_welch_asm_d.py with COUNTED
LOAD WAITS and, as a second switch, STREAMING sample loads.  The arithmetic is variant 44's: the same vector instructions on the same values.

mdsp_welch_w64d_asm starts every unit body with s_waitcnt vmcnt(0), and the 64 loads of the next unit are issued through the tail of the body as
their registers fall free: the last one a dozen instructions before that wait, so every unit parks at its top for most of an HBM miss.  Here
  * no unit body starts with a wait.  In front of the first instruction that touches a register loaded by load n the generator emits
    s_waitcnt vmcnt(k), k = the VMEM operations issued behind load n up to that point (the queue retires in order); a wait an earlier one covers is
    left out.  The counts are found by replaying the loop A B A B until the queue at the top of A repeats (count_waits).  The flush paths end in a
    full wait, and so does the prologue: a queue shorter than the replay's is always safe, since vmcnt(k) then waits for no less;
  * what the waits are worth is the SLACK of a load: the instructions issued between it and the wait that covers it.  Three things raise its
    minimum: the first layer of pass A walks its eight groups in the order N1_ORDER (groups that share operand pairs next to each other); the
    allocator knows until when an operand pair has to be free -- the next unit's first touch of it, less the slack aimed at -- and gives a value the
    free pair with the earliest such deadline that its last use still meets (allocate); and of the loads whose registers are free the one consumed
    first is issued first (merge_loads).  Reached: a least slack of 338 instructions (median 415), variant 44: 12 (median 270); the target was
    200, an HBM miss of ~900 clocks at ~4.5 clocks per packed operation;
  * GenENT (`--nt FILE`), mdsp_welch_w64e_nt_asm: the sample loads carry `nt`: every sample is read once, in whole 256-byte runs, so no line of it
    is worth keeping in L2 or in the Infinity Cache.  The window and twiddle preloads and the row stores stay plain (the rows are read back at
    once).  This switch did not clear its A/B in the headline step (profiles/welch_w64e_ab.json: -0.3 % of the Welch stage, inside the spread), so
    the library does not build that form and its file is not kept; the generator and its checks still cover it.

    python tools/gen_welch_asm_e.py [--check] [--slack] [--nt FILE] [--ablate loads,lds,perm,acc]
        writes dsp.jl_amd/csrc/welch_w64e_asm.s (and, with --nt, the streaming form to FILE); --slack prints the slack figures of that file and of
        welch_w64d_asm.s
Kernel contract: gen_welch_asm_d.py's.
"""
import os
import re
import sys
from collections import deque

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_welch_asm as W
import gen_welch_asm_c as C
import gen_welch_asm_d as D
from gen_welch_asm import Ins, VBASE, keys_of

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsp.jl_amd", "csrc")
SLACK_TARGET = 200     # instructions: an HBM miss of ~900 clocks at ~4.5 clocks per packed operation
VMCNT_MAX = 63         # six bits on gfx9


def touches(ins):
    return {key for o in ins.operands() for key in keys_of(o)}


class GenE(D.GenD):
    NAME = "mdsp_welch_w64e_asm"
    SCRIPT = "tools/gen_welch_asm_e.py"
    TOP_WAIT = False
    N1_ORDER = (0, 1, 2, 3, 4, 5, 6, 7)    # the first layer's groups, first to last; n1 and n1 ^ 1 share the pairs of the compact banks
    # The allocator's deadlines: an operand pair the next unit first touches at instruction t is to be free AIM - t + EARLY instructions before the end
    # of the body (EARLY where t > AIM).  Swept over AIM 200 .. 280 x EARLY 0 .. 600: the least slack is 263 at (240, 0), 302 over most of the range,
    # 338 here with the loads between instructions 1147 and 1606 of 1650 -- where variant 44 has them -- and falls to 205 and below from (280, 160) on:
    # the allocator then no longer finds a pair for every value that meets its deadline.
    AIM = SLACK_TARGET + 80
    EARLY = 140

    def emit_unit(self):
        """GenD's dataflow with the groups of pass A's first layer in N1_ORDER: the list scheduler takes the lowest ready index, so this is its priority"""
        super().emit_unit()
        marks = [k for k, i in enumerate(self.ins) if i.op == "comment"]
        head, sec = self.ins[: marks[0] + 1], self.ins[marks[0] + 1: marks[1]]
        assert len(sec) % 8 == 0
        per = len(sec) // 8
        groups = [sec[per * g: per * (g + 1)] for g in range(8)]
        for g, grp in enumerate(groups):       # a group starts with its window pairs and names no value of another group
            assert grp[0].op == "ds_read_b64" and grp[0].imm == self.WIN_OFF + 512 * g
        self.ins = head + [i for g in self.N1_ORDER for i in groups[g]] + self.ins[marks[1]:]

    def input_units(self):
        """the 64 registers the loads inside a body fill: this unit's bank C and H1"""
        return {key for e in range(32) for key in keys_of(self.cval(self.parity, e))} | {key for g in self.hh_layout() for v in g for key in keys_of(("v", v.p))}

    def first_touch(self):
        """register unit -> index in the scheduled list of the first instruction that touches it, for the registers the PREVIOUS body's loads fill"""
        mine = {key for e in range(32) for key in keys_of(self.cval(1 - self.parity, e))} | {key for g in self.hh_layout() for v in g for key in keys_of(("v", v.p))}
        out = {}
        for k, i in enumerate(self.ins):
            for key in touches(i) & mine:
                out.setdefault(key, k)
        return out

    # ---- register allocation: GenC's, with the choice among the free pairs made by deadline
    def allocate(self, next_touch):
        n = len(self.ins)
        last = {}
        for k, i in enumerate(self.ins):
            for o in i.operands():
                if o[0] in ("v", "h"):
                    last[o[1]] = k
        death = dict(last)
        inputs = self.input_pairs()
        locked = self.bank_pairs(1 - self.parity)
        mine = self.input_units()
        # the next unit's H2 goes into this unit's bank C: its value e is the next unit's bank N value e, touched there with the same group
        deadline = {}
        for p in inputs - locked:
            t = min(next_touch[key] for key in (("p", p, 0), ("p", p, 1)) if key in mine)
            deadline[p] = n - max(0, self.AIM - t) - self.EARLY
        free = [p for p in range(self.POOL0, self.POOL0 + 2 * self.NPOOL, 2) if p not in inputs]
        pmap = {}
        quar = deque()
        live = len(inputs)
        for k, i in enumerate(self.ins):
            while quar and quar[0][0] <= k:
                free.append(quar.popleft()[1])
            for o in i.operands():
                if o[0] in ("v", "h") and o[1] >= VBASE and o[1] not in pmap:
                    if not free:
                        if quar:
                            free.append(quar.popleft()[1])
                        else:
                            raise RuntimeError(f"register pool exhausted at instruction {k}")
                    need = death[o[1]] + 8
                    fit = [q_ for q_ in free if deadline.get(q_, n + 1) >= need]
                    # the earliest deadline this value still meets (a pair that is no operand register has none: the long-lived values end up there)
                    p = min(fit, key=lambda q_: (deadline.get(q_, n + 1), q_)) if fit else max(free, key=lambda q_: (deadline.get(q_, n + 1), -q_))
                    free.remove(p)
                    pmap[o[1]] = p
                    live += 1
                    self.maxlive = max(self.maxlive, live)
            for o in i.operands():
                if o[0] in ("v", "h") and last.get(o[1]) == k:
                    phys = pmap[o[1]] if o[1] >= VBASE else o[1]
                    last[o[1]] = -1
                    if phys in locked:
                        continue
                    if self.POOL0 <= phys < self.POOL0 + 2 * self.NPOOL:
                        quar.append((k + 3, phys))
                        live -= 1

        def ph(o):
            if o is None:
                return None
            if o[0] == "v" and o[1] >= VBASE:
                return ("v", pmap[o[1]])
            if o[0] == "h" and o[1] >= VBASE:
                return ("h", pmap[o[1]], o[2])
            return o
        for i in self.ins:
            i.d = ph(i.d)
            i.s = tuple(ph(o) for o in i.s)

    def merge_loads(self, body, loads, next_touch, gap=4):
        """Gen.merge_loads with one change: of the loads whose destination pair is free, the one the next unit touches first is issued first"""
        last = {}
        for k, i in enumerate(body):
            for o in i.operands():
                if o[0] in ("v", "h"):
                    last[o[1]] = k
        pend = [(last.get(ld.d[1], -1) + gap, next_touch[keys_of(ld.d)[0]], n_, ld) for n_, ld in enumerate(loads) if ld.op == "buffer_load_dword"]
        out = []
        issued = 0
        since = 0
        n = len(body)
        for k, i in enumerate(body):
            out.append(i)
            since += 1
            if not pend:
                continue
            stride = max(1, (n - k) // (len(pend) + 1))
            ready = [t for t in pend if t[0] <= k]
            if ready and since >= min(stride, 6):
                t = min(ready, key=lambda t: t[1:3])
                pend.remove(t)
                out.append(t[3])
                issued += 1
                since = 0
        out.extend(t[3] for t in sorted(pend, key=lambda t: t[1:3]))
        self.loads_in_body = issued
        return out

    @classmethod
    def build_pair(cls):
        gA, gB = cls(0), cls(1)
        for g in (gA, gB):
            g.ins = []
            g.emit_unit()
            g.schedule(64)
        touch = {0: gA.first_touch(), 1: gB.first_touch()}
        bodies = []
        for g in (gA, gB):
            nt = touch[1 - g.parity]
            g.allocate(nt)
            g.insert_waits()
            g.fix_permlane_hazards()
            body = g.ins
            g.ins = []
            g.emit_loads(first=False)
            bodies.append(g.merge_loads(body, list(g.ins), nt))
        bodyA, bodyB = count_waits(*bodies)
        return gA, gB, bodyA, bodyB, cls(0).build_first_loads()


class GenENT(GenE):
    NAME = "mdsp_welch_w64e_nt_asm"
    LOAD_POLICY = " nt"


def count_waits(bodyA, bodyB):
    """s_waitcnt vmcnt(k) in front of the first instruction that touches the destination of a load still in the in-order queue, k = the operations
    behind that load.  The loop is replayed A B A B ... from an empty queue until the queue at the top of A repeats; the bodies of the last trip are
    the kernel's."""
    def one(body, q):
        out = []
        for i in body:
            regs = touches(i)
            need = -1
            for pos, dst in enumerate(q):
                if dst & regs:
                    need = pos
            if need >= 0:
                cnt = min(len(q) - 1 - need, VMCNT_MAX)
                out.append(Ins("s_waitcnt_vm", imm=cnt))
                del q[: len(q) - cnt]
            out.append(i)
            if i.op == "buffer_load_dword":
                q.append(set(keys_of(i.d)))
        return out

    q, seen = [], None
    for _ in range(8):
        top = [sorted(d) for d in q]
        a = one(bodyA, q)
        b = one(bodyB, q)
        if top == seen:
            return a, b
        seen = top
    raise RuntimeError("the load queue at the top of unit A does not settle")


# ------------------------------------------------------------------------------------------------------------------ slack, from an assembly file
_REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def _regs(text):
    out = set()
    for m in _REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def unit_bodies(path):
    """the instruction lines of unit A and unit B of a generated kernel (.LunitX up to .LflushX)"""
    lines = [l.split(";")[0].strip() for l in open(path)]
    out = []
    for tag in "AB":
        a, b = lines.index(f".Lunit{tag}:"), lines.index(f".Lflush{tag}:")
        out.append([l for l in lines[a + 1: b] if l])
    return out


def slack(path):
    """For each of the 64 loads of unit A and of unit B: the instructions issued between the load and the s_waitcnt that covers it, replaying
    A B A B with an in-order queue (s_waitcnt and s_nop lines are not counted as instructions issued).  Returns {"A": [...], "B": [...]} in issue order."""
    A, B = unit_bodies(path)
    q = []              # [destination registers, instructions issued since, tag, number]
    res = {}
    for trip, (tag, body) in enumerate((("A", A), ("B", B), ("A", A), ("B", B))):
        nload = 0
        for line in body:
            m = re.match(r"s_waitcnt vmcnt\((\d+)\)", line)
            if m:
                while len(q) > int(m.group(1)):
                    _, cnt, t_, n_ = q.pop(0)
                    if trip >= 2 or t_ == "B":       # steady state: loads of the second B on are not retired in this replay
                        res.setdefault((t_, n_), cnt)
                continue
            if line.startswith("s_waitcnt") or line.startswith("s_nop"):
                continue
            regs = _regs(line)
            for e in q:
                assert not (e[0] & regs), f"{path}: '{line}' touches the destination of an outstanding load"
                e[1] += 1
            if line.startswith("buffer_load_dword"):
                q.append([_regs(line.split(",")[0]), 0, tag, nload])
                nload += 1
    return {t: [res[(t, n_)] for n_ in range(64)] for t in "AB"}


def slack_summary(path):
    s = slack(path)
    both = s["A"] + s["B"]
    srt = sorted(both)
    return {"min": srt[0], "median": srt[len(srt) // 2], "max": srt[-1], "below_target": sum(1 for x in both if x < SLACK_TARGET), "A": s["A"], "B": s["B"]}


_VREG = re.compile(r"\bv(\d+|\[\d+:\d+\])")


def arithmetic_multiset(path):
    """per unit body: the sorted instruction lines without s_waitcnt and s_nop, without the policy bit of the loads, and with every VGPR number replaced
    by `v`: opcode, modifiers, SGPR operands, LDS and buffer offsets stay.  Equal multisets = the same arithmetic (the allocator renames registers)."""
    out = []
    for body in unit_bodies(path):
        keep = [re.sub(r" nt$", "", l) for l in body if not l.startswith(("s_waitcnt", "s_nop"))]
        out.append(sorted(_VREG.sub("v", l) for l in keep))
    return out


def check():
    return C.check(GenE) and C.check(GenENT)


def kernel_text(G=GenE):
    return C.kernel_text(G)


OUTPUTS = ((GenE, "welch_w64e_asm.s"),)

if __name__ == "__main__":
    if "--check" in sys.argv:
        sys.exit(0 if check() else 1)
    if "--slack" in sys.argv:
        for f in ("welch_w64d_asm.s", "welch_w64e_asm.s"):
            s = slack_summary(os.path.join(CSRC, f))
            print(f"{f}: slack min {s['min']}, median {s['median']}, max {s['max']}, {s['below_target']} of 128 loads below {SLACK_TARGET}")
        sys.exit(0)
    if "--ablate" in sys.argv:
        W.ABLATE.update(sys.argv[sys.argv.index("--ablate") + 1].split(","))
    for G, name in OUTPUTS:
        text, nbody = kernel_text(G)
        out = os.path.join(CSRC, name)
        open(out, "w").write(text)
        print(f"wrote {out}: {text.count(chr(10))} lines, {nbody} instructions per unit")
    if "--nt" in sys.argv:
        out = sys.argv[sys.argv.index("--nt") + 1]
        open(out, "w").write(kernel_text(GenENT)[0])
        print(f"wrote {out}")
