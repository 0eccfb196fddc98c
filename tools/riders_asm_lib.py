"""What tools/gen_riders16_asm.py builds its hand-scheduled wave-step from: instruction records with an issue-cost model (Ins, valu,
trans), register names, and an emitter that inserts the counted waits and pads the hazards the hardware does not interlock.

The schedule itself - MFMA order, register map, fragment rings, the placement of every VALU rider - is the generator's.  (This
module is what is left of the generator of the 32x32x16 riders step, which the 16x16x32 step superseded: DESIGN.md 10.)
"""

MFMA_ISSUE = 8                                            # issue cycles of one MFMA in the cost model
ORD5 = [(1, 0), (0, 0), (1, 1), (0, 1), (0, 2)]           # LDS-fed products (weight part, state part), streamed layout


class Ins:
    __slots__ = ("text", "cost", "reads", "writes", "kind", "ready", "lds_need", "lds_tag", "vm_need", "vm_tag", "accread")

    def __init__(self, text, cost, reads=(), writes=(), kind="valu", ready=-1):
        self.text, self.cost, self.reads, self.writes, self.kind, self.ready = text, cost, set(reads), set(writes), kind, ready
        self.lds_need = self.lds_tag = self.vm_need = self.vm_tag = None
        self.accread = False


def V(n): return "v%d" % n
def A(n): return "a%d" % n
def VQ(n): return "v[%d:%d]" % (n, n + 3)
def AQ(n): return "a[%d:%d]" % (n, n + 3)


def valu(op, dst, *src, cost=4, kind="valu", ready=-1):
    regs = [s for s in src if isinstance(s, int)]
    txt = "%s %s, %s" % (op, V(dst), ", ".join(V(s) if isinstance(s, int) else s for s in src))
    return Ins(txt, cost, ["v%d" % r for r in regs], ["v%d" % dst], kind, ready)


def trans(op, dst, src, ready=-1):
    return valu(op, dst, src, cost=8, kind="trans", ready=ready)


class Emitter:
    """The instruction list of one wave-step.  An Ins may carry a tag for the LDS read / buffer load it issues (lds_tag, vm_tag) and
    the tag of the one it needs (lds_need, vm_need): emit() puts the counted s_waitcnt in front of the consumer and the wait states
    between dependent neighbours."""

    def __init__(self, order23, budget):
        self.budget, self.order23 = budget, order23
        self.out = []                      # emitted Ins
        self.lds_q = []                    # outstanding LDS op tags, in issue order
        self.vm_q = []
        self.stats = {"mfma": 0, "riders": 0, "nops": 0, "waits": 0, "over": 0}

    def emit(self, ins):
        prev = self.out[-1] if self.out else None
        if ins.lds_need is not None and ins.lds_need in self.lds_q:
            newer = len(self.lds_q) - 1 - self.lds_q.index(ins.lds_need)
            self.raw("s_waitcnt lgkmcnt(%d)" % min(newer, 15), 1, "wait")
            keep = min(newer, 15)
            self.lds_q = self.lds_q[len(self.lds_q) - keep:] if keep else []
            prev = self.out[-1]
        if ins.vm_need is not None and ins.vm_need in self.vm_q:
            newer = len(self.vm_q) - 1 - self.vm_q.index(ins.vm_need)
            self.raw("s_waitcnt vmcnt(%d)" % min(newer, 63), 1, "wait")
            keep = min(newer, 63)
            self.vm_q = self.vm_q[len(self.vm_q) - keep:] if keep else []
            prev = self.out[-1]
        # transcendental result -> next VALU: one wait state
        if prev is not None and prev.kind == "trans" and ins.kind in ("valu", "trans", "mfma") and (prev.writes & ins.reads):
            self.raw("s_nop 0", 4, "nop")
        # VALU write -> MFMA A / B operand: two wait states
        if ins.kind == "mfma":
            need = 0
            for back, p in enumerate(reversed(self.out[-2:])):
                if p.kind in ("valu", "trans") and (p.writes & ins.reads):
                    need = max(need, 2 - back)
            if need:
                self.raw("s_nop %d" % (need - 1), 4 * need, "nop")
        self.out.append(ins)
        if ins.lds_tag is not None:
            self.lds_q.append(ins.lds_tag)
        if ins.vm_tag is not None:
            self.vm_q.append(ins.vm_tag)

    def wait_lds(self, tag):
        if tag in self.lds_q:
            newer = len(self.lds_q) - 1 - self.lds_q.index(tag)
            self.raw("s_waitcnt lgkmcnt(%d)" % min(newer, 15), 1, "wait")
            keep = min(newer, 15)
            self.lds_q = self.lds_q[len(self.lds_q) - keep:] if keep else []

    def raw(self, text, cost, kind):
        self.out.append(Ins(text, cost, kind=kind))
        self.stats["nops" if kind == "nop" else "waits"] += 1
