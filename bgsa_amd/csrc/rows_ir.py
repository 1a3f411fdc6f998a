#!/usr/bin/env python3
"""rows_ir.py — the DP row bodies of the gfx950 kernels as a tiny instruction-level IR.

One description of each algorithm's row update serves two consumers:

  * emit_asm():  gfx950 assembly text for the inline-asm row loops (gen_rows_asm.py), and
  * simulate():  a numpy interpreter of the very same instruction list, so the instruction
                 stream that ships can be checked bit-for-bit against the oracle on a CPU
                 (tests/test_rows_ir.py) before it ever runs on a GPU.

BGSA's reference emits its kernels from a generator as well (generator/source/src/main/java/org/
sduhpcl/bgsa/generator/{MyersGenerator,BitPAlGenerator}.java); this is the gfx950 counterpart.

Instruction selection follows scripts/ubench/valu_rate.hip, measured on MI355X:
  fast class (~2.2 cycles per wave64 instruction): v_and/v_or/v_xor/v_not/v_mov/v_add_u32,
      v_bitop3_b32 (any 3-input boolean), and the 4-byte VOP2 forms of v_add_co/v_addc_co that
      carry through VCC;
  slow class (~4.2 cycles, and they drag neighbouring fast instructions down with them):
      v_lshlrev/v_lshrrev, v_alignbit, v_lshl_or, v_and_or, v_or3, v_bfi, v_add3, v_bcnt, v_cmp and
      every VOP3 form that reads or writes an SGPR-pair carry.
Operand count also has a price (scripts/ubench/bank_conflict.hip): a stream of nothing but three-VGPR-
source v_bitop3 issues at ~2.95 cycles against ~2.27 for two-source VOP2 or for the two alternating;
the VGPR bank (index mod 4) of the sources makes no difference, a run of 8-byte VOP3 encodings with two
sources sits in between (~2.6).  In the 75-instruction BitPAl body of the time (49 of them three-source) turning
every v_bitop3 into a two-source instruction would buy 6.5 %, in the Myers planes body 3 % — the
instruction count is the lever, so two-source forms are used only where they cost no extra instruction.
So every 1-bit shift across words is an add-with-carry chain (x + x + carry), every chain goes
through VCC, and chains are serialised into phases.  gfx950 hazard "VALU writes VCC -> VALU reads
VCC as carry-in: 2 wait states" is enforced by the emitter (it counts the instructions between the
links of a chain and pads with s_nop if an ordering ever leaves fewer than two).
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, field

import numpy as np


def _knob(name: str, default: str) -> str:
    """A build-time switch of the generators: the environment's BGSA_GEN_<name>, read once when this file is imported."""
    return os.environ.get(f"BGSA_GEN_{name}", default)


CLASS_CODE = np.zeros(256, dtype=np.uint8)      # the alphabet map of original/BGSA_CPU/global.c:9-15, as a byte table for arrays:
CLASS_CODE[list(b"ACGTN")] = range(5)           # A C G T N = 0..4, every other character 0


def class_code(ch) -> int:
    """The class of one query character."""
    return int(CLASS_CODE[int(ch)])


def _low_mask(bits: int) -> np.uint32:
    """The lowest `bits` bits of a word (none below 1, all from 32 on): the columns of a word that belong to the subject."""
    return np.uint32(0xFFFFFFFF if bits >= 32 else (0 if bits <= 0 else (1 << bits) - 1))


def tt(fn) -> int:
    """Truth table immediate of v_bitop3_b32 for a boolean function of (a, b, c)."""
    return fn(0xF0, 0xCC, 0xAA) & 0xFF


TT_XOR3 = tt(lambda a, b, c: a ^ b ^ c)
TT_MAJ = tt(lambda a, b, c: (a & b) | (a & c) | (b & c))
TT_OR3 = tt(lambda a, b, c: a | b | c)
TT_NOR3 = tt(lambda a, b, c: ~(a | b | c))


@dataclass
class Op:
    kind: str                 # and or xor not mov bitop3 add_co addc setc1
    dst: str = ""
    srcs: tuple = ()
    imm: int = 0
    dst2: str = ""            # second destination (shr64: the low word of the pair)


@dataclass
class Body:
    """Straight-line row body.  Register names: 'S<i>' persistent state (updated in place),
    'E<j>' the match masks of the current query character, 'P<n>' a FIXED register of the emitting loop (P<2i> / P<2i+1> = the
    low / high word of aligned pair i, for the 64-bit instructions; they keep their value from row to row), anything else is a
    temporary."""
    ops: list = field(default_factory=list)

    def _emit(self, kind, dst, *srcs, imm=0):
        self.ops.append(Op(kind, dst, tuple(srcs), imm))
        return dst

    def AND(self, d, a, b): return self._emit("and", d, a, b)
    def OR(self, d, a, b): return self._emit("or", d, a, b)
    def XOR(self, d, a, b): return self._emit("xor", d, a, b)
    def NOT(self, d, a): return self._emit("not", d, a)
    def MOV(self, d, a): return self._emit("mov", d, a)
    def BITOP3(self, d, a, b, c, fn): return self._emit("bitop3", d, a, b, c, imm=tt(fn))
    def ADD_CO(self, d, a, b): return self._emit("add_co", d, a, b)   # d = a + b, VCC = carry out
    def ADDC(self, d, a, b): return self._emit("addc", d, a, b)       # d = a + b + VCC, VCC = carry out
    def SETC1(self): return self._emit("setc1", "")                    # VCC = all ones (carry-in 1)
    # A wave has ONE fast carry register (VCC; the VOP3 forms with an SGPR-pair carry are slow class).  A chain is parked in a
    # scalar pair '$c<n>' and taken up again later (s_mov_b64: scalar pipe, no VALU issue slot) — what lets two chains run
    # over the words in turns instead of one after the other (myers_body(split=K)).
    def SAVECC(self, slot): return self._emit("savecc", f"$c{slot}")    # $c<slot> = VCC
    def LOADCC(self, slot): return self._emit("loadcc", "", f"$c{slot}")  # VCC = $c<slot>
    # The same through a VECTOR register, two fast-class VALU instructions instead of two scalar moves that wait for the vector
    # pipe: d = 0 - VCC (v_subb_co_u32 d, vcc, d, d, vcc: all ones where the carry is set; d's old value cancels), and
    # VCC = carry of d + d (v_add_co_u32 d, vcc, d, d; d is dead afterwards).
    def SAVEV(self, d): return self._emit("savev", d)                    # d = VCC ? ~0 : 0   (VCC left undefined)
    def LOADV(self, d): return self._emit("loadv", d, d)                 # VCC = d's top bit  (d clobbered)

    def ADDCZ(self, d): return self._emit("addcz", d, d)              # d = d + VCC  (v_addc_co_u32 d, vcc, 0, d, vcc)
    def SUBBZ(self, d): return self._emit("subbz", d, d)              # d = d - VCC  (v_subbrev_co_u32 d, vcc, 0, d, vcc)
    def MINU(self, d, a, b): return self._emit("minu", d, a, b)       # d = min(a, b), unsigned

    def ADD(self, d, a, b): return self._emit("add", d, a, b)          # d = a + b, no carry
    def LSHR1(self, d, a): return self._emit("lshr1", d, a)            # d = a >> 1 (slow class)
    def ALIGNBIT(self, d, hi, lo, sh): return self._emit("alignbit", d, hi, lo, sh)  # ({hi,lo} >> sh)[31:0], sh scalar
    def LSHRS(self, d, a, sh): return self._emit("lshrs", d, a, sh)   # d = a >> sh, sh scalar (VOP2 v_lshrrev_b32: fast class)
    def LSHL_IMM(self, d, a, n): return self._emit("lshl_imm", d, a, imm=n)   # d = a << n, n an immediate (slow class)

    def SHR64(self, hi, lo):
        """{hi, lo} >>= 1 as ONE v_lshrrev_b64 on an aligned register pair (P<2i+1>, P<2i>): hi's bit 0 arrives in lo's bit 31."""
        self.ops.append(Op("shr64", hi, (hi, lo), 0, lo))
        return hi

    def MATCH3(self, d, b0, b1, b2, wild=False):
        """d = columns whose 3-bit character code (b2 b1 b0) equals the row's class (0..4 = A C G T
        N): a v_bitop3 whose truth table depends on which of the five body copies it sits in.
        wild: code 7, which no character has, matches every class (the semi-global kernels' unused low
        columns) — still one instruction, only the truth tables differ."""
        tts = tuple(tt(lambda x0, x1, x2, c=c: ((x0 if c & 1 else ~x0) & (x1 if c & 2 else ~x1) & (x2 if c & 4 else ~x2))
                       | ((x0 & x1 & x2) if wild else 0))
                    for c in range(5))
        return self._emit("match3", d, b0, b1, b2, imm=tts)

    # ---- analysis ---------------------------------------------------------------------------
    def temps(self) -> list[str]:
        seen = []
        for op in self.ops:
            for r in (op.dst, op.dst2) + op.srcs:
                if r and not r.startswith(("S", "E", "B", "$", "P")) and r not in seen:
                    seen.append(r)
        return seen

    def allocate_temps(self) -> tuple[dict, int]:
        """Linear-scan reuse of temporaries: name -> slot, and the number of slots needed."""
        last_use = {}
        for i, op in enumerate(self.ops):
            for r in (op.dst,) + op.srcs:
                if r and not r.startswith(("S", "E", "B", "$", "P")):
                    last_use[r] = i
        slot_of, free, n_slots = {}, [], 0
        for i, op in enumerate(self.ops):
            # sources die at their last use, before the destination of this op is placed only if
            # the hardware reads operands before writing (it does: dst may alias a dying source)
            dying = sorted({r for r in op.srcs if r in slot_of and last_use[r] == i and r != op.dst})
            for r in dying:
                free.append(slot_of[r])
            d = op.dst
            if d and not d.startswith(("S", "E", "B", "$", "P")) and d not in slot_of:
                if free:
                    slot_of[d] = free.pop()
                else:
                    slot_of[d] = n_slots
                    n_slots += 1
            if d and d in slot_of and last_use.get(d, -1) == i:  # written, never read
                free.append(slot_of[d])
        return slot_of, n_slots

    def valu_count(self) -> int:
        return sum(op.kind not in ("setc1", "savecc", "loadcc") for op in self.ops)

    def salu_count(self) -> int:
        return sum(op.kind in ("setc1", "savecc", "loadcc") for op in self.ops)

    # ---- numpy interpreter --------------------------------------------------------------------
    def simulate(self, state: list, eq: list, cls: int = 0, planes: list | None = None,
                 scalars: dict | None = None, fixed: dict | None = None) -> None:
        """state: list of uint32 arrays (updated in place); eq: match masks of the row's class
        ('E' registers); planes: the class-independent 'B' registers; cls: the row's class; fixed: the 'P' registers, which keep
        their values between rows (the caller's dict, updated in place)."""
        regs: dict[str, np.ndarray] = {}
        fixed = {} if fixed is None else fixed
        vcc = np.zeros_like(state[0], dtype=bool)
        parked: dict[str, np.ndarray] = {}     # carry chains parked in scalar pairs (savecc / loadcc)

        def rd(name):
            if name.startswith("S"):
                return state[int(name[1:])]
            if name.startswith("E"):
                return eq[int(name[1:])]
            if name.startswith("B"):
                return planes[int(name[1:])]
            if name.startswith("$"):
                return np.full_like(state[0], scalars[name])
            if name.startswith("P"):
                return fixed[name]
            return regs[name]

        def wr(name, val):
            val = val.astype(np.uint32)
            if name.startswith("S"):
                state[int(name[1:])] = val
            elif name.startswith("P"):
                fixed[name] = val
            else:
                regs[name] = val

        FULL = np.uint32(0xFFFFFFFF)
        for op in self.ops:
            k = op.kind
            if k == "setc1":
                vcc = np.ones_like(vcc)
                continue
            if k == "savecc":
                parked[op.dst] = vcc.copy()
                continue
            if k == "loadcc":
                vcc = parked[op.srcs[0]].copy()
                continue
            if k == "savev":
                wr(op.dst, np.where(vcc, FULL, np.uint32(0)))
                vcc = vcc.copy()      # the borrow out of d - d - VCC equals VCC: the chain's carry survives, nothing relies on it
                continue
            if k == "loadv":
                d = rd(op.srcs[0])
                vcc = (d >> np.uint32(31)) != 0
                wr(op.dst, (d.astype(np.uint64) * np.uint64(2)) & np.uint64(0xFFFFFFFF))
                continue
            s = [rd(x) for x in op.srcs]
            if k == "and": wr(op.dst, s[0] & s[1])
            elif k == "or": wr(op.dst, s[0] | s[1])
            elif k == "xor": wr(op.dst, s[0] ^ s[1])
            elif k == "not": wr(op.dst, s[0] ^ FULL)
            elif k == "mov": wr(op.dst, s[0])
            elif k == "add": wr(op.dst, (s[0].astype(np.uint64) + s[1].astype(np.uint64)) & np.uint64(0xFFFFFFFF))
            elif k == "lshr1": wr(op.dst, s[0] >> np.uint32(1))
            elif k == "lshrs": wr(op.dst, s[0] >> s[1].astype(np.uint32))
            elif k == "lshl_imm": wr(op.dst, (s[0].astype(np.uint64) << np.uint64(op.imm)) & np.uint64(0xFFFFFFFF))
            elif k == "alignbit":
                pair = (s[0].astype(np.uint64) << np.uint64(32)) | s[1].astype(np.uint64)
                wr(op.dst, (pair >> s[2].astype(np.uint64)) & np.uint64(0xFFFFFFFF))
            elif k in ("bitop3", "match3"):
                a, b, c = s
                imm = op.imm if k == "bitop3" else op.imm[cls]
                out = np.zeros_like(a)
                for idx in range(8):
                    if (imm >> idx) & 1:
                        ta = a if idx & 4 else a ^ FULL
                        tb = b if idx & 2 else b ^ FULL
                        tc = c if idx & 1 else c ^ FULL
                        out |= ta & tb & tc
                wr(op.dst, out)
            elif k in ("add_co", "addc"):
                wide = s[0].astype(np.uint64) + s[1].astype(np.uint64)
                if k == "addc":
                    wide = wide + vcc.astype(np.uint64)
                vcc = (wide >> np.uint64(32)) != 0
                wr(op.dst, wide & np.uint64(0xFFFFFFFF))
            elif k == "addcz":
                wide = s[0].astype(np.uint64) + vcc.astype(np.uint64)
                vcc = (wide >> np.uint64(32)) != 0
                wr(op.dst, wide & np.uint64(0xFFFFFFFF))
            elif k == "subbz":
                borrow = vcc & (s[0] == 0)
                wr(op.dst, (s[0].astype(np.int64) - vcc.astype(np.int64)) & np.int64(0xFFFFFFFF))
                vcc = borrow
            elif k == "minu": wr(op.dst, np.minimum(s[0], s[1]))
            elif k == "shr64":
                pair = ((s[0].astype(np.uint64) << np.uint64(32)) | s[1].astype(np.uint64)) >> np.uint64(1)
                wr(op.dst, pair >> np.uint64(32))
                wr(op.dst2, pair & np.uint64(0xFFFFFFFF))
            else:
                raise ValueError(k)

    # ---- gfx950 assembly ------------------------------------------------------------------------
    def emit_asm(self, reg_name, cls: int = 0) -> list[str]:
        """reg_name(name) -> asm operand text; cls = character class of this body copy.
        Returns instruction lines with hazard padding."""
        lines: list[str] = []
        since_vcc_write = 99  # instructions issued since the last write of VCC
        for op in self.ops:
            k = op.kind
            if k == "setc1":
                lines.append("s_mov_b64 vcc, -1")
                since_vcc_write = 0
                continue
            if k == "savecc":      # a scalar read of VCC behind the VALU write: interlocked by the hardware
                lines.append(f"s_mov_b64 {reg_name(op.dst)}, vcc")
                since_vcc_write += 1
                continue
            if k == "loadcc":      # treated like setc1: its reader keeps two instructions' distance
                lines.append(f"s_mov_b64 vcc, {reg_name(op.srcs[0])}")
                since_vcc_write = 0
                continue
            if k == "savev":       # a VALU read of VCC: the chain link's two wait states
                if since_vcc_write < 2:
                    lines.append(f"s_nop {1 - since_vcc_write}")
                d = reg_name(op.dst)
                lines.append(f"v_subb_co_u32 {d}, vcc, {d}, {d}, vcc")
                since_vcc_write = 0
                continue
            if k == "loadv":
                d = reg_name(op.dst)
                lines.append(f"v_add_co_u32 {d}, vcc, {d}, {d}")
                since_vcc_write = 0
                continue
            r = [reg_name(x) for x in op.srcs]
            d = reg_name(op.dst)
            if k in ("addc", "addcz", "subbz") and since_vcc_write < 2:
                lines.append(f"s_nop {1 - since_vcc_write}")
                since_vcc_write = 2
            if k == "and": lines.append(f"v_and_b32 {d}, {r[0]}, {r[1]}")
            elif k == "or": lines.append(f"v_or_b32 {d}, {r[0]}, {r[1]}")
            elif k == "xor": lines.append(f"v_xor_b32 {d}, {r[0]}, {r[1]}")
            elif k == "not": lines.append(f"v_not_b32 {d}, {r[0]}")
            elif k == "mov": lines.append(f"v_mov_b32 {d}, {r[0]}")
            elif k == "add": lines.append(f"v_add_u32 {d}, {r[0]}, {r[1]}")
            elif k == "lshr1": lines.append(f"v_lshrrev_b32 {d}, 1, {r[0]}")
            elif k == "alignbit": lines.append(f"v_alignbit_b32 {d}, {r[0]}, {r[1]}, {r[2]}")
            elif k == "lshrs": lines.append(f"v_lshrrev_b32 {d}, {r[1]}, {r[0]}")
            elif k == "lshl_imm": lines.append(f"v_lshlrev_b32 {d}, {op.imm}, {r[0]}")
            elif k == "bitop3": lines.append(f"v_bitop3_b32 {d}, {r[0]}, {r[1]}, {r[2]} bitop3:0x{op.imm:02x}")
            elif k == "match3": lines.append(f"v_bitop3_b32 {d}, {r[0]}, {r[1]}, {r[2]} bitop3:0x{op.imm[cls]:02x}")
            elif k == "add_co": lines.append(f"v_add_co_u32 {d}, vcc, {r[0]}, {r[1]}")
            elif k == "addc": lines.append(f"v_addc_co_u32 {d}, vcc, {r[0]}, {r[1]}, vcc")
            elif k == "addcz": lines.append(f"v_addc_co_u32 {d}, vcc, 0, {r[0]}, vcc")
            elif k == "subbz": lines.append(f"v_subbrev_co_u32 {d}, vcc, 0, {r[0]}, vcc")
            elif k == "minu": lines.append(f"v_min_u32 {d}, {r[0]}, {r[1]}")
            elif k == "shr64":
                h, l = reg_name(op.srcs[0]), reg_name(op.srcs[1])
                assert h[0] == "v" and l[0] == "v" and int(h[1:]) == int(l[1:]) + 1 and int(l[1:]) % 2 == 0, (h, l)
                lines.append(f"v_lshrrev_b64 v[{l[1:]}:{h[1:]}], 1, v[{l[1:]}:{h[1:]}]")
            else:
                raise ValueError(k)
            since_vcc_write = 0 if k in ("add_co", "addc", "addcz", "subbz") else since_vcc_write + 1
        return lines


def count_hazard_nops(body: "Body") -> int:
    """s_nop padding emit_asm() would insert: addc issued fewer than 2 instructions after a VCC write."""
    nops, since = 0, 99
    for op in body.ops:
        if op.kind in ("setc1", "loadcc"):
            since = 0
            continue
        if op.kind == "savecc":
            since += 1
            continue
        if op.kind == "loadv":
            since = 0
            continue
        if op.kind in ("addc", "addcz", "subbz", "savev") and since < 2:
            nops += 1
            since = 2
        since = 0 if op.kind in ("add_co", "addc", "addcz", "subbz", "savev") else since + 1
    return nops


def schedule(body: "Body", window: int = 48) -> "Body":
    """List-schedule a straight-line body so that carry chains keep moving and the two wait states
    between the links of a chain are filled with independent work instead of s_nop.

    Dependencies: read-after-write, write-after-read and write-after-write on every register name
    and on VCC (add_co / setc1 write it, addc reads and writes it), so chains stay intact and never
    interleave.  Priority: the next chain link as soon as it is hazard-free; otherwise the earliest
    instruction in program order that does not read VCC.  `window` bounds how far ahead of the oldest
    unscheduled instruction a filler may be taken from — it trades nops against live registers."""
    ops = body.ops
    n = len(ops)
    last_write: dict = {}
    readers: dict = {}
    preds = [set() for _ in range(n)]
    for i, op in enumerate(ops):
        reads = [r for r in op.srcs if r]
        writes = [w for w in (op.dst, op.dst2) if w]
        if op.kind in ("addc", "addcz", "subbz", "savecc", "savev"):
            reads.append("VCC")
        if op.kind in ("add_co", "addc", "setc1", "addcz", "subbz", "loadcc", "savev", "loadv"):
            writes.append("VCC")
        for r in reads:
            if r in last_write:
                preds[i].add(last_write[r])
        for w in writes:
            if w in last_write:
                preds[i].add(last_write[w])
            preds[i].update(readers.get(w, ()))
        for r in reads:
            readers.setdefault(r, []).append(i)
        for w in writes:
            last_write[w] = i
            readers[w] = []
        preds[i].discard(i)
    succs = [[] for _ in range(n)]
    for i in range(n):
        for p in preds[i]:
            succs[p].append(i)
    remaining = [len(preds[i]) for i in range(n)]
    done = [False] * n
    ready = sorted(i for i in range(n) if remaining[i] == 0)
    order = []
    since = 99
    oldest = 0
    while len(order) < n:
        while oldest < n and done[oldest]:
            oldest += 1
        cands = [i for i in ready if i < oldest + window] or ready[:1]
        chain = [i for i in cands if ops[i].kind in ("addc", "add_co", "setc1", "addcz", "subbz")]
        plain = [i for i in cands if ops[i].kind not in ("addc", "addcz", "subbz")]
        if since >= 2 and chain:
            pick = chain[0]                      # the chain is the critical path: keep it moving
        elif since < 2 and plain:
            nonchain = [i for i in plain if ops[i].kind not in ("add_co", "setc1")]
            pick = (nonchain or plain)[0]        # a wait state to fill
        else:
            pick = cands[0]                      # nothing to fill it with: emit_asm() pads with s_nop
        ready.remove(pick)
        done[pick] = True
        order.append(pick)
        since = 0 if ops[pick].kind in ("add_co", "addc", "setc1", "addcz", "subbz") else since + 1
        for s in succs[pick]:
            remaining[s] -= 1
            if remaining[s] == 0:
                ready.append(s)
        ready.sort()
    out = Body()
    out.ops = [ops[i] for i in order]
    return out


def _dependencies(ops):
    """Per op the (predecessor, kind) pairs of a straight-line op list: 'raw' = reads what the predecessor wrote (a true
    dependency: the value has to exist), 'vcc' = the same through the carry register, 'order' = write-after-read /
    write-after-write (only the order matters)."""
    last_write: dict = {}
    readers: dict = {}
    deps = [[] for _ in ops]
    for i, op in enumerate(ops):
        reads = [(r, "raw") for r in op.srcs if r]
        writes = [w for w in (op.dst, op.dst2) if w]
        if op.kind in ("addc", "addcz", "subbz", "savecc", "savev"):
            reads.append(("VCC", "vcc"))
        if op.kind in ("add_co", "addc", "setc1", "addcz", "subbz", "loadcc", "savev", "loadv"):
            writes.append("VCC")
        if op.kind == "savev":
            reads = [x for x in reads if x[1] == "vcc"]      # d's old value cancels: not a dependency
        for r, kind in reads:
            if r in last_write:
                deps[i].append((last_write[r], kind))
        for w in writes:
            if w in last_write:
                deps[i].append((last_write[w], "order"))
            deps[i] += [(j, "order") for j in readers.get(w, ()) if j != i]
        for r, _ in reads:
            readers.setdefault(r, []).append(i)
        for w in writes:
            last_write[w] = i
            readers[w] = []
    return deps


def schedule_ilp(body: "Body", gap: int = 1, window: int = 24, vcc_dist: int = 3) -> "Body":
    """List-schedule a straight-line body so that no instruction issues right behind the one whose result it reads.

    Why (round 5): the Myers rows are, as written, ONE dependent chain — a = VP & E feeds the add, the add feeds HN, HN feeds M2,
    M2 feeds HP — and a gfx950 SIMD issues a wave's dependent instruction later than an independent one.  With eight waves per
    SIMD the other waves fill the slots; at two waves (the 1000 bp kernels: 228-253 VGPRs) they cannot, and every scalar
    instruction or wait in the loop shows in the time (0.877 of the issue peak against 0.93-0.98 at 150 bp).  Here every true
    dependency keeps `gap` other instructions between producer and consumer where the body has independent work to put there;
    carry links keep the two the hardware demands (VALU writes VCC -> VALU reads VCC: 2 wait states); a chain parked by SAVECC
    (a scalar read of VCC) waits `gap` + 1.  Among the instructions that may issue, the one with the longest dependent path
    behind it goes first (the carry chains are the critical path); `window` bounds how far ahead of the oldest unscheduled
    instruction one may be taken from — it trades stalls against live temporaries."""
    ops = body.ops
    n = len(ops)
    deps = _dependencies(ops)
    need = {"raw": gap + 1, "vcc": max(3, vcc_dist), "order": 1}   # vcc_dist: instructions from one carry link to the next (>= 3: two wait states)
    succs = [[] for _ in range(n)]
    for i in range(n):
        for p_, _ in deps[i]:
            succs[p_].append(i)
    height = [1] * n
    for i in range(n - 1, -1, -1):
        for s_ in succs[i]:
            height[i] = max(height[i], 1 + height[s_])
    remaining = [len({p_ for p_, _ in deps[i]}) for i in range(n)]
    pos = [None] * n
    ready = [i for i in range(n) if remaining[i] == 0]
    order = []
    oldest = 0
    done = [False] * n
    while len(order) < n:
        while oldest < n and done[oldest]:
            oldest += 1
        here = len(order)

        def earliest(i):
            t = 0
            for p_, kind in deps[i]:
                # a scalar read of VCC (SAVECC) has no wait states to keep, but it stalls its wave until the vector pipe has
                # delivered the carry: keep gap + 1 instructions between it and the link it reads
                d = gap + 2 if (ops[i].kind == "savecc" and kind == "vcc") else need[kind]
                t = max(t, pos[p_] + d)
            return t

        cands = [i for i in ready if i < oldest + window] or [min(ready)]
        free = [i for i in cands if earliest(i) <= here]
        if free:
            pick = max(free, key=lambda i: (height[i], -i))
        else:
            pick = min(cands, key=lambda i: (earliest(i), -height[i], i))
        ready.remove(pick)
        done[pick] = True
        pos[pick] = here
        order.append(pick)
        for s_ in set(succs[pick]):
            remaining[s_] -= 1
            if remaining[s_] == 0:
                ready.append(s_)
    out = Body()
    out.ops = [ops[i] for i in order]
    return out


def dependent_pairs(body: "Body") -> int:
    """How many instructions read a register the instruction right before them wrote (VALU results only)."""
    n = 0
    for prev, op in zip(body.ops, body.ops[1:]):
        if prev.kind in ("setc1", "savecc", "loadcc") or op.kind in ("setc1", "savecc", "loadcc"):
            continue
        if prev.dst and prev.dst in op.srcs:
            n += 1
    return n


# =================================================================================================
# Myers unit-cost global (reference original/BGSA_CPU/align_core.c:65-132)
# =================================================================================================

MYERS_EIGHT = _knob('MYERS_EIGHT', '1') != '0'   # '0': the 10-instruction rows of rounds 1-3 (A/B builds)


def _state(first: int = 0):
    """Names of VP and VN of word w where the rows' state starts at word `first` of the S registers."""
    return (lambda w: f"S{(first + w) * 2}"), (lambda w: f"S{(first + w) * 2 + 1}")


def _plane_mask(b: Body, name: str, wild: bool = False):
    """The match mask of word w rebuilt from its code planes B[3w..3w+2] (MATCH3) into the temporary `name` ('{w}' = the word)."""
    return lambda w: b.MATCH3(name.format(w=w), f"B{w * 3}", f"B{w * 3 + 1}", f"B{w * 3 + 2}", wild)


def _myers_eight(b: Body, nw: int, VP, VN, mask, a: str = "a{w}", m: str = "m{w}", split: int = 0, balanced: bool = False,
                 edge: int = 1, tap=(None, None), park=None, place=()) -> None:
    """THE eight-instruction Myers cell (myers_body's docstring), appended to `b` for `nw` words: every eight-instruction body
    is a call of this.  Per word
        phase A:  a = VP & E ; m = VP + a (chain 0) ; a = HNs = m ^ VP ^ a ; m = M2 = E | VN | HNs ; VP = HP = VN | ~(M2 | VP)
        phase B:  VP = HP + HP (chain 1) ; VN = M2 & HPs ; VP = (M2 & HNs) | ~(M2 | HPs)
    VP(w), VN(w): the state registers; mask(w): the register that holds word w's match mask (it may emit the instruction
    that forms it: _plane_mask); a, m: the names of the two temporaries, '{w}' = the word.  The names are part of the
    emitted text's contract — allocate_temps frees in name order, the schedulers run on the named ops.
    split = K > 0, balanced: see myers_body.
    edge: the row edge D[i][0] - D[i-1][0], chain 1's carry-in into HP at bit 0 of word 0.  1 (global): a SETC1, and every link
    of the chain is an ADDC; 0 (semi-global): the chain's first link is an ADD_CO, as chain 0's always is.
    tap[c]: a call that reads the carry LEAVING chain c behind its last link (SUBBZ / ADDCZ into a running score), or None.
    park = (save, load): how a pausing chain waits between the blocks, save(c) / load(c); the default is a scalar pair.
    place: where the chain ends sit, all of them behind an instruction of a block's LAST word.  The events, in the order they
    are emitted where two share a place:
        park0  save chain 0 (not in the last block)                   tap0  tap[0] (last block)
        take1  chain 1's carry: the edge's SETC1 in the first block, load(1) afterwards
        park1  save chain 1 (not in the last block)                   tap1  tap[1] (last block)
        take0  load chain 0 (not in the last block)
    and the places: 'sum', 'hn', 'm2', 'hp' = behind that instruction of phase A ('hp' is the phase's end also where balanced
    forms HP later), 'ahead' = two instructions in front of phase A's end ('sum' where balanced leaves the word's HP to
    phase B, else 'hn'), 'shift', 'vn', 'vp' = behind that instruction of phase B.  The hazard padding and the schedulers see
    this order, so every caller states the one it has always had."""
    A, M = (lambda w: a.format(w=w)), (lambda w: m.format(w=w))
    save, load = park or (b.SAVECC, b.LOADCC)
    place = {"park0": "sum", "tap0": "m2", "take1": "ahead", "park1": "shift", "tap1": "vn", "take0": "vn", **dict(place)}
    hp = lambda w: b.BITOP3(VP(w), M(w), VN(w), VP(w), lambda m_, vn, vp: (m_ & vn) | ~(m_ | vp))
    blocks = [(0, nw)] if split <= 0 else [(lo, min(nw, lo + split)) for lo in range(0, nw, split)]
    for j, (lo, hi) in enumerate(blocks):
        first, last = j == 0, j == len(blocks) - 1
        ahead = "sum" if balanced and hi - lo > 1 else "hn"

        def at(here, w):
            for ev in ("park0", "tap0", "take1", "park1", "tap1", "take0"):
                if w != hi - 1 or here != (ahead if place[ev] == "ahead" else place[ev]):
                    continue
                c = int(ev[-1])
                if ev.startswith("park") and not last:
                    save(c)
                elif ev.startswith("tap") and last and tap[c]:
                    tap[c]()
                elif ev == "take1" and first and edge:
                    b.SETC1()
                elif ev.startswith("take") and not (first if c else last):
                    load(c)

        for w in range(lo, hi):      # phase A: the addition's carry chain
            e = mask(w)
            b.AND(A(w), VP(w), e)
            (b.ADDC if w else b.ADD_CO)(M(w), VP(w), A(w))
            at("sum", w)
            b.BITOP3(A(w), M(w), VP(w), A(w), lambda s_, vp, a_: s_ ^ vp ^ a_)
            at("hn", w)
            b.BITOP3(M(w), e, VN(w), A(w), lambda e_, vn, hn: e_ | vn | hn)
            at("m2", w)
            if not balanced or w == lo:
                hp(w)
            at("hp", w)
        for w in range(lo, hi):      # phase B: HP << 1 across words, then the new deltas
            (b.ADDC if w or edge else b.ADD_CO)(VP(w), VP(w), VP(w))
            if balanced and w + 1 < hi:
                hp(w + 1)
            at("shift", w)
            b.AND(VN(w), M(w), VP(w))
            at("vn", w)
            b.BITOP3(VP(w), M(w), A(w), VP(w), lambda m_, hn, hp_: (m_ & hn) | ~(m_ | hp_))
            at("vp", w)


def _myers_ten(b: Body, nw: int, P, M, mask, d: str = "d{w}", hp: str = "hp{w}", hn: str | None = None,
               edge: int = 1, tap=(None, None), early: int = 0) -> None:
    """THE ten-instruction Myers cell of rounds 1-3 (BGSA_GEN_MYERS_EIGHT=0 builds it; full 32-bit words, hardware carries
    instead of the reference's software carry bit, align_core.c:79-83,91-96), appended to `b` for `nw` words:
        phase A:  D0 = (((P & E) + P) ^ P) | E | M                    (the addition's chain)
        phase C:  HP = ~(D0 | P) | M ; HN = D0 & P ; HP <<= 1         (the HP shift's chain, carry-in = edge)
        phase D:  HN <<= 1 (its chain) ; M' = D0 & HP ; P' = ~(D0 | HP) | HN
    P(w), M(w): the state registers VP, VN; mask(w), edge as in _myers_eight; d, hp, hn: the temporaries' names, hn = None: HN
    is parked in the P register between the phases (nine registers per word instead of ten).
    tap = (behind phase C, behind phase D): calls that read the carry leaving the HP / the HN shift, or None.
    early = n: the new M of the first n words is formed behind phase C, so that tap[0] keeps two instructions' distance from
    the chain's last link."""
    D, HP = (lambda w: d.format(w=w)), (lambda w: hp.format(w=w))
    HN = P if hn is None else (lambda w: hn.format(w=w))
    new_m = lambda w: b.AND(M(w), D(w), HP(w))
    for w in range(nw):  # phase A: the addition's carry chain
        e = mask(w)
        b.AND(D(w), P(w), e)   # (P & (E|M)) == (P & E): P & M == 0 is an invariant
        (b.ADDC if w else b.ADD_CO)(D(w), D(w), P(w))
        b.BITOP3(D(w), D(w), P(w), M(w), lambda a, p, m: (a ^ p) | m)
        b.OR(D(w), D(w), e)
    if edge:
        b.SETC1()  # D[i][0] - D[i-1][0] = +1 enters HP at bit 0 of word 0
    for w in range(nw):  # phase C: HP << 1 across words
        b.BITOP3(HP(w), D(w), P(w), M(w), lambda d_, p, m: ~(d_ | p) | m)
        b.AND(HN(w), D(w), P(w))
        (b.ADDC if w or edge else b.ADD_CO)(HP(w), HP(w), HP(w))
    for w in range(min(early, nw)):
        new_m(w)
    if tap[0]:
        tap[0]()
    for w in range(nw):  # phase D: HN << 1 across words, then the new vertical deltas
        (b.ADDC if w else b.ADD_CO)(HN(w), HN(w), HN(w))
        if w >= early:
            new_m(w)
        b.BITOP3(P(w), D(w), HP(w), HN(w), lambda d_, hp_, hn_: ~(d_ | hp_) | hn_)
    if tap[1]:
        tap[1]()


def myers_body(nw: int, groups: int = 1, split: int = 0, park: str = "sgpr", balanced: bool = False) -> Body:
    """State layout: S[(g*nw + w)*2 + 0] = VP word w of group g, +1 = VN.  E[g*nw + w] = match mask.

    Per word EIGHT instructions and two carry chains (round 4; ten and three until then: myers_body10).  In the terms of the
    general-scores body (u = 1 - dH in {0, 1, 2}: VP = [u = 0], VN = [u = 2]; v = 1 - dV likewise) a cell is m = max(W, u, v_in),
    v = m - u, new u = m - v_in with W = 2 at a match, 1 otherwise — so m is ONE bit, M2 = [m = 2] = E | VN | [v_in = 2], and
    [v_in = 2] of column j + 1 is VP_j & M2_j = (VP_j & E_j) | (VP_j & [v_in = 2]_j): a carry with generate VP & E and propagate
    VP, i.e. the carries of the addition VP + (VP & E), and the carry INTO a bit is sum ^ VP ^ (VP & E) — [v_in = 2] comes out of
    the adder already moved up one column, across the words.  What the classical order pays for (HN and its shift) is gone:
        a = VP & E ; s = VP + a (chain, carry-in 0) ; HNs = s ^ VP ^ a ; M2 = E | VN | HNs ; HP = VN | ~(M2 | VP)
        HPs = HP << 1 (chain, carry-in 1: the row edge) ; VN' = M2 & HPs ; VP' = (M2 & HNs) | ~(M2 | HPs)
    (reference: 24 ops per 31-bit word, align_core.c:72-103).  Two temporaries per word: HP is formed in the dead VP register.

    split = K > 0 (round 5): the two chains take turns over blocks of K words instead of running over all the words one after
    the other — phase A of words 0..K-1, phase B of the same words, phase A of K..2K-1, ... — with the chain that pauses parked
    in a scalar pair (SAVECC / LOADCC, scalar pipe).  The two temporaries of a word then live for one block, not for the row:
    2K temporaries instead of 2*nw, which is what lets 30 and 32 words keep their five Peq planes resident (7*nw + 2K + the
    kernel's own registers <= 256) where they ran on the code planes, nine instructions per word, before.
    park = "vgpr": the pausing chain waits in a vector register (SAVEV / LOADV: one fast-class VALU instruction each, two more
    temporaries) instead of a scalar pair — a scalar move of VCC waits for the vector pipe to drain, and at two waves per
    SIMD nobody fills the gap.
    balanced: HP of word w + 1 is formed in phase B, between the shift of word w and its new deltas, instead of at the end of
    phase A — four instructions from carry link to carry link in BOTH phases where the order above has five and three."""
    if not MYERS_EIGHT:
        return myers_body10(nw, groups)
    b = Body()
    for g in range(groups):
        # A scalar pair hands chain 1 its carry two instructions ahead of its reader (the defaults); a vector register is read two
        # instructions behind the link that wrote it (a VALU read of VCC) and, as written, loaded right in front of its reader:
        # schedule_ilp, or the emitter's s_nop, spaces them
        vgpr = dict(park=(lambda c: b.SAVEV(f"cv{g}_{c}"), lambda c: b.LOADV(f"cv{g}_{c}")),
                    place={"park0": "m2", "take1": "hp", "park1": "vp", "take0": "vp"}) if park == "vgpr" else {}
        _myers_eight(b, nw, *_state(g * nw), lambda w: f"E{g * nw + w}", f"a{g}_{{w}}", f"m{g}_{{w}}", split, balanced, **vgpr)
    return b


# ---- certified diagonal band -------------------------------------------------------
# A path through cell (i, j) of the m x n matrix holds at least |d| + |d - (n - m)| indels, d = j - i.  A pair whose distance
# is <= B therefore has its optimal paths inside the band |d| + |d - (n - m)| <= B, and a row only needs the words that touch
# the band's columns.  Words left of the row's window keep their last deltas (the lowest active word gets the row-edge
# carry-ins: D[i][edge] = D[i-1][edge] + 1, a vertical step), words right of it keep their initial state (a horizontal
# path): every column still holds the cost of a real path, so the score D' >= D, and D' <= B certifies D' = D.
MYERS_BAND_MAX_WORDS = 8      # widths with windowed bodies (myers_band_rows_asm): 65..256 bp


def myers_window_body(nw: int, a: int, b: int, groups: int = 1, balanced: bool = False) -> Body:
    """myers_body(b - a + 1) on state words a..b of an nw-word row (S/E registers renumbered): the row-edge carry-ins
    (0 into the addition, 1 into the HP shift) enter at word a.
    groups = G > 1: the same window of G subject groups, one after the other, registers laid out as myers_body(nw, G) lays
    them out — S[(g*nw + w)*2], E[g*nw + w].  Each group's two carry chains stay whole: they share VCC, which orders them, so
    a scheduler can only move the other group's chain-free instructions into a chain's wait states."""
    assert 0 <= a <= b < nw and groups >= 1
    src = myers_body(b - a + 1, balanced=balanced)
    out = Body()
    for g in range(groups):
        def ren(x: str) -> str:
            if x.startswith("S"):
                return f"S{int(x[1:]) + 2 * (g * nw + a)}"
            if x.startswith("E"):
                return f"E{int(x[1:]) + g * nw + a}"
            if g and x and not x.startswith("$"):      # the temporaries a0_<w>, m0_<w> of the one-group body
                return f"{x[0]}{g}{x[2:]}"
            return x

        out.ops += [Op(op.kind, ren(op.dst), tuple(ren(s) for s in op.srcs), op.imm, op.dst2) for op in src.ops]
    return out


def myers_window_index(nw: int, a: int, b: int) -> int:
    """Slot group of window [a, b] in myers_band_rows_asm: the windows a <= b < nw in lexicographic order."""
    return a * nw - a * (a - 1) // 2 + (b - a)


def myers_band_half(length: int) -> int:
    """Default half-width h (B = 2h + 1) for subjects / queries of `length`: the mean edit distance of random uniform
    ACGT pairs plus 4.5 standard deviations (20,000 pairs per length, 65..256 bp, LABNOTES §11).  Same formula as
    myers_global.hip: band_default_half."""
    return (9 * length + 192) // 32


def myers_band_rescue_half(length: int) -> int:
    """Half-width of a launch that scores its uncertified lanes again one by one (myers_band.h: band_rescue_half): three
    below the default, where about one random pair in a thousand lies above B (LABNOTES §33)."""
    return myers_band_half(length) - 3


# Early leave (myers_band.h: kBandEarlyCuts): per length the cuts (row r, word w) — behind row r the window begins at word w + 1.
MYERS_BAND_EARLY_CUTS = {
    68: ((51, 0),),
    96: ((60, 0), (83, 1)),
    100: ((62, 0), (85, 1)),
    107: ((64, 0), (88, 1)),
    111: ((65, 0), (89, 1)),
    114: ((66, 0), (90, 1)),
    118: ((67, 0), (92, 1)),
    121: ((68, 0), (93, 1)),
    125: ((69, 0), (94, 1)),
    128: ((70, 0), (95, 1)),
    132: ((71, 0), (96, 1)),
    139: ((99, 1), (121, 2)),
    143: ((100, 1), (122, 2)),
    146: ((101, 1), (123, 2)),
    150: ((106, 1), (130, 2)),
    153: ((104, 1), (126, 2)),
    157: ((105, 1), (128, 2)),
    160: ((106, 1), (129, 2)),
}


def myers_band_early_cuts(length: int, h: int):
    """The table's cuts for length x length at half-width h (myers_band.h: band_early_cuts): only at the rescue half-width."""
    return MYERS_BAND_EARLY_CUTS.get(length, ()) if h == myers_band_rescue_half(length) else ()


def myers_band_windows(m: int, n: int, h: int, nw: int, cuts=()):
    """Per query row i = 1..m the window (a, b) of words that holds the band's columns, or None when the band is off for
    this shape (the row windows would not save a fifth of the word-rows, or |n - m| leaves no room).  Same rule as
    myers_global.hip: band_schedule.  cuts = ((r, w), ...), n = m: rows i > r run on windows that begin at word w + 1 or later
    (myers_band.h: band_schedule_early); None where a cut is out of order, has r < 32 (w + 1) or empties a window."""
    if cuts:
        base = myers_band_windows(m, n, h, nw)
        cuts = list(cuts)
        if base is None or m != n or len(cuts) > 2 or any(not (0 <= w < nw - 1 and 32 * (w + 1) <= r < m) for r, w in cuts) or \
                any(x[0] >= y[0] or x[1] >= y[1] for x, y in zip(cuts, cuts[1:])):
            return None
        out = [(max([a] + [w + 1 for r, w in cuts if i > r]), b) for i, (a, b) in enumerate(base, start=1)]
        return None if any(a > b for a, b in out) else out
    B = 2 * h + 1
    delta = n - m
    if h <= 0 or abs(delta) > B or nw > MYERS_BAND_MAX_WORDS or nw < 3:
        return None
    dlo, dhi = -((B - delta) // 2), (delta + B) // 2        # ceil((delta - B) / 2), floor((delta + B) / 2)
    out = []
    for i in range(1, m + 1):
        jlo, jhi = max(1, i + dlo), min(n, i + dhi)
        out.append(((jlo - 1) // 32, (jhi - 1) // 32))
    if 5 * sum(b - a + 1 for a, b in out) > 4 * m * nw:
        return None
    return out


def myers_band_stream(codes, m: int, n: int, h: int, nw: int, cuts=()) -> bytes | None:
    """The band stream of one query (codes: m class codes 0..4): the plain stream's row codes, END and REFILL, plus
    SETWIN (7) and a window byte wherever the row's window changes; a SETWIN never straddles a REFILL (a REFILL at byte 6
    ends the window early).  One spare all-END window follows.  Restates myers_global.hip: band_stream_layout.
    cuts (early leave): on the windows of myers_band_windows(cuts = cuts)."""
    win = myers_band_windows(m, n, h, nw, cuts) if cuts else myers_band_windows(m, n, h, nw)
    if win is None:
        return None
    out = bytearray()

    def refill():
        out.append(6)
        while len(out) % 8:
            out.append(5)

    def put(c):
        if len(out) % 8 == 7:
            refill()
        out.append(c)

    cur = None
    for i in range(m):
        if win[i] != cur:
            if len(out) % 8 >= 6:
                refill()
            out += bytes([7, myers_window_index(nw, *win[i])])
            cur = win[i]
        put(int(codes[i]))
    put(5)
    while len(out) % 8:
        out.append(5)
    out += bytes([5] * 8)
    return bytes(out)


def myers_band_segments(codes, m: int, n: int, h: int, nw: int, depths, cuts=()) -> tuple[bytes, list] | None:
    """The stream of one query cut behind rows depths[0] < depths[1] < ... (prefix sharing): one band stream per
    segment — it begins with the SETWIN of its first row's window whether or not the window changes there, ends with END
    padded to its 8-byte window, and only the last one carries the spare all-END window.  Returns the bytes and the offsets
    of the segments followed by the total length.  None where the band is off or a row up to the deepest depth leaves
    words 0..1.  Restates myers_band.h: band_rows_layout / prefix_plan_layout.
    cuts (early leave): on the windows of myers_band_windows(cuts = cuts)."""
    win = myers_band_windows(m, n, h, nw, cuts) if cuts else myers_band_windows(m, n, h, nw)
    depths = list(depths)
    if win is None or not depths or depths != sorted(set(depths)) or depths[0] < 1 or depths[-1] >= m:
        return None
    if any(w not in ((0, 0), (0, 1)) for w in win[:depths[-1]]):
        return None
    out, offsets = bytearray(), []
    cuts = [0] + depths + [m]
    for j in range(len(cuts) - 1):
        offsets.append(len(out))
        seg = bytearray()
        cur = None
        for i in range(cuts[j], cuts[j + 1]):
            if win[i] != cur:
                if len(seg) % 8 >= 6:
                    seg += bytes([6] + [5] * (7 - len(seg) % 8))
                seg += bytes([7, myers_window_index(nw, *win[i])])
                cur = win[i]
            if len(seg) % 8 == 7:
                seg.append(6)
            seg.append(int(codes[i]))
        if len(seg) % 8 == 7:
            seg.append(6)
        seg.append(5)
        seg += bytes([5] * (-len(seg) % 8))
        if j == len(cuts) - 2:
            seg += bytes([5] * 8)
        out += seg
    offsets.append(len(out))
    return bytes(out), offsets


def run_band_stream(nw: int, state: list, peq: np.ndarray, stream: bytes, band: bool = True, balanced: bool = False,
                    schedule=None, groups: int = 1) -> int:
    """Interpret a band stream the way myers_band_rows_asm walks it (band = False: SETWIN keeps the full window; schedule:
    the pass the generator applies to every body, gen_rows_asm.ilp); returns the number of word-rows executed (per group).  groups = G: state and peq hold the
    G groups of one wave, myers_body(nw, G)'s layout (peq[c, g*nw + w])."""
    windows = [(a, b) for a in range(nw) for b in range(a, nw)]
    bodies = {}
    cur = (0, nw - 1)
    pos, rows = 0, 0
    while True:
        c = stream[pos]
        if c == 5:
            return rows
        if c == 6:
            pos = (pos | 7) + 1
            continue
        if c == 7:
            k = stream[pos + 1]
            assert k < len(windows) and myers_window_index(nw, *windows[k]) == k
            cur = windows[k] if band else (0, nw - 1)
            pos += 2
            continue
        assert c < 5
        if cur not in bodies:
            bodies[cur] = myers_window_body(nw, *cur, groups=groups, balanced=balanced)
            if schedule is not None:
                bodies[cur] = schedule(bodies[cur])
        bodies[cur].simulate(state, [peq[c, w] for w in range(groups * nw)], cls=c)
        rows += cur[1] - cur[0] + 1
        pos += 1


def run_band_early(nw: int, peq: np.ndarray, codes, m: int, h: int, cuts, groups: int = 1, **kw):
    """One query over its early-leave stream the way the RESCUE kernels certify it (myers_global.hip): behind cut (r, w) no row
    touches words 0 .. w, so behind the last row they still hold D'[r][j_r] - r, j_r = 32 (w + 1), and the lane's limit is the
    least of B and every cut's M = D'[r][j_r] + (r - j_r).  Returns (scores D' [groups][lanes], limits [groups][lanes],
    word-rows); a lane is certified by D' <= limit."""
    lanes = peq.shape[2]
    state = myers_init_state(nw, groups, lanes)
    rows = run_band_stream(nw, state, peq, myers_band_stream(codes, m, m, h, nw, cuts), groups=groups, **kw)
    limit = [np.full(lanes, 2 * h + 1, dtype=np.int64) for _ in range(groups)]
    for r, w in cuts:
        for g in range(groups):
            limit[g] = np.minimum(limit[g], 2 * r - 32 * (w + 1) + _myers_columns(state[2 * g * nw:], w + 1, 32 * (w + 1)))
    return [m + _myers_columns(state[2 * g * nw:], nw, m) for g in range(groups)], limit, rows


def myers_body10(nw: int, groups: int = 1) -> Body:
    """The ten-instruction row (_myers_ten) in myers_body's layout: S[(g*nw + w)*2 + 0] = VP word w of group g, +1 = VN,
    E[g*nw + w] = match mask; the row boundary feeds 1 into the HP shift."""
    b = Body()
    for g in range(groups):
        _myers_ten(b, nw, *_state(g * nw), lambda w: f"E{g * nw + w}", f"d{g}_{{w}}", f"hp{g}_{{w}}", f"hn{g}_{{w}}")
    return b


def myers_semi_body(nw: int, split: int = 0) -> Body:
    """Semi-global Myers (generator -m 0 -s, MyersGenerator.java:56-223): the subject end to end inside the
    query — D[i][0] = 0 for every query row i, result = min over i of D[i][n].  The body is myers_body with
      * carry-in 0 instead of 1 for the HP shift (the row edge D[i][0] - D[i-1][0] = 0), and
      * the subject RIGHT-ALIGNED in its words (the kernel shifts the masks once per task; the unused low
        columns match every character and start at VP = 0, so they stay at D = 0 and hand the row edge to
        the first real column), which puts the last subject column at bit 31 of the last word: the carries
        that leave the HP and HN shift chains ARE D[i][n] - D[i-1][n], added to / subtracted from the running
        score with one add-with-carry each, plus one v_min for the best score — 3 instructions per row on top of
        the 10 per word, nothing extracted bit by bit.
    State: myers_body's, then S[2nw] = D[i][n] (running), S[2nw+1] = its minimum so far.
    split = K > 0: the two chains in turns over blocks of K words, as myers_body(split=K) — 2K temporaries, which keeps the five Peq
    planes resident up to 32 words (round 5); the two carries that leave the chains are taken where the LAST block's phases end."""
    return _myers_semi_rows(nw, lambda b: (lambda w: f"E{w}"), "hn{w}", split)


def _myers_semi_rows(nw: int, mask, hn: str | None, split: int = 0) -> Body:
    """myers_semi_body and myers_semi_planes_body behind their match masks (mask(b) is the cell's `mask`; hn: _myers_ten's).
    Eight instructions: the carry that LEAVES the addition chain is [v = 2] of the last column = its HN bit, the one that leaves
    the HP shift its HP bit — 8 VALU per word + 3 per row; both are taken where the LAST block's phases end, the HN bit two
    instructions behind the chain's last link (and in front of the other chain's LOADCC), the HP bit before anything else
    writes VCC.  Ten instructions (never split): the HP bit behind phase C, the HN bit behind phase D."""
    b = Body()
    RUN, BEST = f"S{2 * nw}", f"S{2 * nw + 1}"
    less, more = (lambda: b.SUBBZ(RUN)), (lambda: b.ADDCZ(RUN))      # - the HN bit, + the HP bit that left the last column
    if MYERS_EIGHT:
        _myers_eight(b, nw, *_state(), mask(b), split=split, edge=0, tap=(less, more), place={"take1": "m2"})
    else:
        _myers_ten(b, nw, *_state(), mask(b), hn=hn, edge=0, tap=(more, less), early=2)
    b.MINU(BEST, BEST, RUN)
    return b


def semi_align(peq: np.ndarray, slen: int, nw: int):
    """What the semi-global kernels do to a subject's match masks once per task: right-align the slen columns
    in nw words and make the unused low columns match everything.  Returns (aligned peq [5][nw][n], VP init
    per word [nw] — 0 in the unused columns, 1 in the subject's).  peq may be any stack [planes][words][n] of per-column
    bits: the code planes are aligned the same way, all ones = code 7 in their unused columns."""
    s = 32 * nw - slen
    assert s >= 0
    planes, words, n = peq.shape
    out = np.zeros((planes, nw, n), dtype=np.uint32)
    vp = []
    for w in range(nw):
        lo_col = 32 * w - s                    # source column of bit 0 of aligned word w
        word = np.zeros((planes, n), dtype=np.uint64)
        for src in (lo_col // 32, lo_col // 32 + 1):
            if 0 <= src < words:
                shift = 32 * src - lo_col      # where source word `src` starts within the aligned word
                v = peq[:, src].astype(np.uint64)
                word |= (v << np.uint64(shift)) if shift >= 0 else (v >> np.uint64(-shift))
        dummy = _low_mask(s - 32 * w)
        out[:, w] = ((word & np.uint64(0xFFFFFFFF)) | np.uint64(dummy)).astype(np.uint32)
        vp.append(~dummy)
    return out, vp


def _semi_state(vp0: list, n: int, slen: int) -> list:
    """Row 0 of the semi-global bodies: VP as semi_align gives it, VN = 0, D[0][n] = n running and as the best so far."""
    st = []
    for vp in vp0:
        st += [np.full(n, vp, np.uint32), np.zeros(n, np.uint32)]
    return st + [np.full(n, slen, np.uint32), np.full(n, slen, np.uint32)]


def myers_semi_simulate(subjects: np.ndarray, query: np.ndarray, nw: int, body: "Body | None" = None) -> np.ndarray:
    """One query against the subjects with myers_semi_body (or the given form of it), set up as myers_semi_asm_kernel<NW> does."""
    n, slen = subjects.shape
    peq, vp0 = semi_align(build_peq32(subjects, (slen + 31) // 32), slen, nw)
    st = _semi_state(vp0, n, slen)
    body = myers_semi_body(nw) if body is None else body
    for ch in query:
        body.simulate(st, list(peq[class_code(ch)]))
    return (-st[2 * nw + 1].astype(np.int64)).astype(np.int16)


def myers_planes_body(nw: int, split: int = 0, balanced: bool = False) -> Body:
    """Myers for long subjects (769..1024 bp): the five Peq planes of a subject (5*nw registers)
    are replaced by its 3-bit character code planes B[w*3+i] (3*nw registers) and the match mask
    of the row's class is rebuilt per word with one v_bitop3 (MATCH3) — 11 instructions per word,
    7*nw+1 registers, which keeps 32 words (1024 bp) at two waves per SIMD.  State as myers_body.
    split = K > 0: the chains in turns over blocks of K words (see myers_body): 5*nw + 2K + 1 registers.
    """
    # a mask name per word: no false dependency between the words' masks (the slots are reused)
    return _myers_planes_rows(nw, "e{w}" if MYERS_EIGHT else "e", split, balanced)


def _myers_planes_rows(nw: int, e: str, split: int = 0, balanced: bool = False) -> Body:
    """myers_planes_body with its match mask in the temporary `e` ('{w}' = the word)."""
    b = Body()
    if MYERS_EIGHT:      # myers_body's eight instructions + the match mask: 9 per word, the same 7*nw + 1 registers
        _myers_eight(b, nw, *_state(), _plane_mask(b, e), split=split, balanced=balanced,
                     place={"take1": "hn" if split > 0 else "sum"})
    else:                # HN parks in the VP register; the new VN (needs only D and the shifted HP) is computed in phase D so that
        #                  every link has two instructions behind it
        _myers_ten(b, nw, *_state(), _plane_mask(b, e))
    return b


def myers_semi_planes_body(nw: int) -> Body:
    """Semi-global Myers for subjects of 769..1024 bp: myers_planes_body with myers_semi_body's changes — HP shift
    with carry-in 0, the subject right-aligned, the carries leaving the HP / HN chains accumulated into the running
    last-column score — and the unused low columns coded 7 in the planes, the code that matches every class (MATCH3
    wild), so they cost no instruction.  9 VALU per word + 3 per row (11 + 3 under the ten-instruction row).
    State: S[2w] = VP, S[2w+1] = VN, S[2nw] = D[i][n], S[2nw+1] = its minimum so far."""
    return _myers_semi_rows(nw, lambda b: _plane_mask(b, "e", wild=True), None)


def myers_semi_planes_simulate(subjects: np.ndarray, query: np.ndarray, nw: int) -> np.ndarray:
    """One query against the subjects with myers_semi_planes_body, set up as myers_semi_planes_kernel<NW> does."""
    n, slen = subjects.shape
    peq = build_peq32(subjects, (slen + 31) // 32)
    planes, vp0 = semi_align(np.stack([peq[1] | peq[3], peq[2] | peq[3], peq[4]]), slen, nw)      # code_planes' three bits
    B = [planes[i, w] for w in range(nw) for i in range(3)]
    st = _semi_state(vp0, n, slen)
    body = myers_semi_planes_body(nw)
    for ch in query:
        body.simulate(st, [], cls=class_code(ch), planes=B)
    return (-st[2 * nw + 1].astype(np.int64)).astype(np.int16)


def myers_block_body(nw: int) -> Body:
    """myers_planes_body for one column block of a subject longer than 1024 bp.  The three carry
    chains enter and leave the block through registers that hold 32 rows' worth of carry bits,
    first row in bit 31:  x + x  shifts the next row's carry-in into VCC,  x + x + vcc  appends
    the row's carry-out — six extra fast-class instructions per row, no bit extraction.
    State: S[2w] = VP, S[2w+1] = VN, then CIN_S, CIN_P, CIN_N, COUT_S, COUT_P, COUT_N."""
    return _myers_blocked(_myers_planes_rows(nw, "e"), nw)      # one mask name for all words, as this body has always had


def _myers_blocked(body: Body, nw: int) -> Body:
    """make_blocked on the kernel's three carry-word pairs.  Chains: addition (carry-in 0), HP shift (carry-in 1 in the first
    block: the row edge), and under the ten-instruction row the HN shift (0); the eight-instruction row's two chains — the
    addition's carries are [v_in = 2] — leave the third pair unused."""
    body, init = make_blocked(body, 2 * nw, n_slots=3)
    assert init == ([0, 1] if MYERS_EIGHT else [0, 1, 0])
    return schedule(body, 16)   # fills the slots around the carry-word instructions


def myers_peq_block_body(nw: int) -> Body:
    """Column-block form of myers_body (Peq planes resident, 8 VALU per word + 4 for the carry words; 10 + 6 until round 4),
    derived mechanically like the BitPAl block bodies."""
    return _myers_blocked(myers_body(nw, 1), nw)


def myers_blocked_simulate(subjects: np.ndarray, query: np.ndarray, nw_block: int, peq_resident: bool = False) -> np.ndarray:
    """A subject processed as column blocks of nw_block words with the block body, carries
    exchanged through per-32-row words exactly as myers_blocked_kernel does.  Returns int16.
    peq_resident: the block body built on myers_body (match masks in registers) instead of the code planes."""
    n, slen = subjects.shape
    qlen = len(query)
    n_blocks = -(-((slen + 31) // 32) // nw_block)
    peq = build_peq32(subjects, n_blocks * nw_block)      # zero masks beyond the subject
    planes_all = code_planes(peq)
    # carry words per 32-row chunk: addition carry-in 0, HP carry-in 1 (row edge), HN carry-in 0
    carry = [[np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32)] for _ in range((qlen + 31) // 32)]
    body = myers_peq_block_body(nw_block) if peq_resident else myers_block_body(nw_block)
    score = np.full(n, qlen, dtype=np.int64)
    for blk in range(n_blocks):
        st = myers_init_state(nw_block, 1, n)
        lo, hi = blk * nw_block, (blk + 1) * nw_block
        if peq_resident:
            row = lambda c: body.simulate(st, list(peq[c, lo:hi]))
        else:
            row = lambda c: body.simulate(st, [], cls=c, planes=planes_all[3 * lo:3 * hi])
        _run_block(row, st, carry, query)
        score += _myers_columns(st, nw_block, slen - 32 * lo)
    return (-score).astype(np.int16)


def _run_block(row, st: list, carry: list, query) -> None:
    """The rows of one column block under the blocked kernels' carry scheme (myers_blocked_kernel, bitpal_blocked_kernel): the
    block's carry-in words (chunk 0's) and as many carry-out words are appended to its state `st`; at every 32nd row — the
    stream's CARRY event — the carry-out words are stored for the block to the right and the chunk's carry-in words taken; a
    partial last chunk is left-aligned.  carry[chunk][chain] is read and replaced; row(c) runs one row of class c on st."""
    base, n_ch = len(st), len(carry[0])
    st += [x.copy() for x in carry[0]] + [np.zeros_like(x) for x in carry[0]]
    for r, ch in enumerate(query):
        if r > 0 and r % 32 == 0:
            carry[r // 32 - 1] = [x.copy() for x in st[base + n_ch:]]
            st[base:base + n_ch] = [x.copy() for x in carry[r // 32]]
        row(class_code(ch))
    tail = len(query) % 32
    carry[-1] = [x << np.uint32(32 - tail) if tail else x.copy() for x in st[base + n_ch:]]     # left-align a partial chunk


def code_planes(peq: np.ndarray) -> list:
    """[5][nw][n] Peq -> class-independent code planes B[w*3+i] (A=0 C=1 G=2 T=3 N=4)."""
    nw = peq.shape[1]
    out = []
    for w in range(nw):
        out += [peq[1, w] | peq[3, w], peq[2, w] | peq[3, w], peq[4, w]]
    return out


def myers_init_state(nw: int, groups: int, lanes: int) -> list:
    st = []
    for _ in range(groups * nw):
        st += [np.full(lanes, 0xFFFFFFFF, dtype=np.uint32), np.zeros(lanes, dtype=np.uint32)]
    return st


def myers_score(state: list, nw: int, qlen: int, slen: int, group: int = 0) -> np.ndarray:
    return (-(qlen + _myers_columns(state[2 * group * nw:], nw, slen))).astype(np.int16)


def _myers_columns(state: list, nw: int, cols: int) -> np.ndarray:
    """D[m][cols] - D[m][0] read off the vertical deltas of the first `cols` columns of nw words (VP, VN pairs)."""
    total = np.zeros(state[0].shape, dtype=np.int64)
    for w in range(nw):
        mask = _low_mask(cols - 32 * w)
        total += np.bitwise_count(state[2 * w] & mask).astype(np.int64) - np.bitwise_count(state[2 * w + 1] & mask).astype(np.int64)
    return total


# =================================================================================================
# Banded Myers (reference banded/BGSA_CPU/align_core.c:19-67, one row of cpu_cal_D0 + cpu_cal_score)
# =================================================================================================

def banded_body() -> Body:
    """32-bit band word (k <= 15).  State: S0 = VP, S1 = VN, S2 = errors counted on the lowest
    diagonal since row k.  E0, E1 = the two words of the row's class match string (offset by k+1
    bits) that the window straddles; scalars: $sh = row mod 32, $mask = band mask, $one = 1.

    The window is one funnel shift of the match string by the row number — the reference shifts
    five windows and feeds each a bit, every row (align_core.c:35-62).  Two slow-class
    instructions remain (the funnel shift and D0 >> 1); everything else is fast class.
    """
    b = Body()
    _banded_row(b, b.ALIGNBIT("w", "E1", "E0", "$sh"), lambda i: f"S{i}", lambda name: name, "d0")
    return b


def _banded_row(b: Body, w: str, S, t, d: str) -> None:
    """The sliding 32-bit row behind its window register w (banded_body: a funnel shift, banded_cut_body: a plain one).
    S(0..2) = VP, VN, errors; t(name): the temporaries' names; d: D0's."""
    b.BITOP3(t("x"), w, "$mask", S(1), lambda w_, m, vn: (w_ & m) | vn)
    b.AND(t("t"), t("x"), S(0))
    b.ADD(t("t"), t("t"), S(0))
    b.BITOP3(d, t("t"), S(0), t("x"), lambda t_, vp, x: (t_ ^ vp) | x)
    b.BITOP3(t("hp"), d, S(0), S(1), lambda d_, vp, vn: ~(d_ | vp) | vn)
    b.AND(t("hn"), d, S(0))
    b.LSHR1(t("x2"), d)
    b.AND(S(1), t("x2"), t("hp"))
    b.BITOP3(S(0), t("hp"), t("x2"), t("hn"), lambda hp, x2, hn: ~(hp | x2) | hn)
    b.BITOP3(t("e"), d, "$one", "$one", lambda d_, one, _o: ~d_ & one)
    b.ADD(S(2), S(2), t("e"))


def banded_body64_sh64(g: int = 0) -> Body:
    """banded_body64 with D0 >> 1 as ONE v_lshrrev_b64 on the fixed pair (P<2g+1> : P<2g>) = (D0 hi : D0 lo) in place of the funnel
    shift and the plain shift: 21 VALU per row; everything else — the error count included — as banded_body64."""
    b = Body()
    dl, dh = f"P{2 * g}", f"P{2 * g + 1}"
    ops = banded_body64().ops
    err_bit = next(op for op in ops if op.dst == "e")      # reads D0's low word: before the in-place shift
    for op in ops:
        if op is err_bit:
            continue
        if op.kind == "alignbit" and op.dst == "x2l":
            b.ops.append(Op(err_bit.kind, "e", (dl,) + err_bit.srcs[1:], err_bit.imm))
            b.SHR64(dh, dl)
            continue
        if op.kind == "lshr1" and op.dst == "x2h":
            continue
        ren = lambda r: {"dl": dl, "dh": dh, "x2l": dl, "x2h": dh}.get(r, r)
        b.ops.append(Op(op.kind, ren(op.dst), tuple(ren(x) for x in op.srcs), op.imm))
    return b


def banded_funnel_body(groups: int = 1, wide: bool = False, sh64: bool = False) -> Body:
    """The funnel-shift rows (banded_body: k <= 15, banded_body64: k <= 31) for one or two subject groups per wave that share
    the stream and its scalar work, interleaved instruction by instruction as banded_cut_body's: group g's state is
    S<n*g .. n*g + n - 1> (n = 3: VP, VN, errors; wide n = 5: VP lo/hi, VN lo/hi, errors), its match-string words
    E<m*g .. m*g + m - 1> (m = 2, wide 3).  groups = 1 is banded_body() / banded_body64() itself.
    sh64: banded_body64_sh64 (its fixed register pair is per group already)."""
    n_state, n_eq = (5, 3) if wide else (3, 2)
    per = []
    for g in range(groups):
        if sh64:
            assert wide
            base = banded_body64_sh64(g)
        else:
            base = banded_body64() if wide else banded_body()
        ops = []
        for op in base.ops:
            def rename(r, g=g):
                if r.startswith("S"):
                    return f"S{n_state * g + int(r[1:])}"
                if r.startswith("E"):
                    return f"E{n_eq * g + int(r[1:])}"
                if r.startswith(("$", "P")):
                    return r
                return f"{r}_{g}"
            ops.append(Op(op.kind, rename(op.dst) if op.dst else "", tuple(rename(x) for x in op.srcs), op.imm,
                          rename(op.dst2) if op.dst2 else ""))
        # units of the interleave: single instructions, and a carry chain (add_co followed by its addc links) as ONE
        # unit — two groups' chains must not interleave, VCC is one register
        units = []
        for op in ops:
            if op.kind == "addc":
                units[-1].append(op)
            else:
                units.append([op])
        per.append(units)
    out = Body()
    for units in zip(*per):
        for u in units:
            out.ops.extend(u)
    return out


def banded_cut_rows(k: int) -> int:
    """Rows between two cuts of the one-word window form (bgsa_common.h: banded_cut_rows): the band's 2k + 1 bits,
    offset by up to rows - 1 bits, must fit one 32-bit word.  0: no room worth it (k > 12) — the funnel-shift row."""
    return 16 if k <= 8 else (8 if k <= 12 else 0)


def banded_cut_body(groups: int = 1) -> Body:
    """The sliding row WITHOUT its funnel shift (k <= 12), for one or two subject groups per wave.

    scripts/ubench/gen_banded_mix.py on MI355X (profiles/r03_ubench_banded_mix.txt): ONE half-rate-class instruction
    in a row makes the whole row issue at ~4.2 cycles per instruction instead of ~2.2 — banded_body's row costs 52.8
    cycles of vector issue with its v_alignbit and 28.4 with a v_mov in its place — and v_alignbit is in that class
    with any kind of shift operand, while v_lshrrev_b32 is not (by an immediate, a VGPR, or — among other
    instructions — an SGPR).  So the window of a row must come out of ONE register: the kernel keeps, per class, the
    32 bits of the match string that start at the last multiple of banded_cut_rows(k) rows ("cut": one v_alignbit
    per class every 16 rows for k <= 8, every 8 for k <= 12, in an event) and the row shifts that word right by
    `row mod cut` — at most cut - 1, which leaves the band's 2k + 1 bits inside the word.  Every instruction of the
    row is then fast class.  E<g> = group g's cut word of the row's class; state S<3g..3g+2> = VP, VN, errors.
    groups = 2: two subject groups share the wave (and the stream's scalar work); their rows are interleaved
    instruction by instruction, two independent dependency chains."""
    per = []
    for g in range(groups):
        b = Body()
        t = lambda name, g=g: f"{name}{g}"
        _banded_row(b, b.LSHRS(t("w"), f"E{g}", "$sh"), lambda i, g=g: f"S{3 * g + i}", t, t("d"))
        per.append(b.ops)
    out = Body()
    for ops in zip(*per):
        out.ops.extend(ops)
    return out


def banded_body64() -> Body:
    """64-bit band (16 <= k <= 31) as register pairs.  State: S0/S1 = VP lo/hi, S2/S3 = VN lo/hi,
    S4 = errors since row k.  E0..E2 = three consecutive 32-bit words of the class match string;
    scalars $sh, $mask_lo, $mask_hi, $one.  22 VALU per row, four of them slow class."""
    b = Body()
    b.ALIGNBIT("wl", "E1", "E0", "$sh")
    b.ALIGNBIT("wh", "E2", "E1", "$sh")
    b.BITOP3("xl", "wl", "$mask_lo", "S2", lambda w, m, vn: (w & m) | vn)
    b.BITOP3("xh", "wh", "$mask_hi", "S3", lambda w, m, vn: (w & m) | vn)
    b.AND("tl", "xl", "S0")
    b.AND("th", "xh", "S1")
    b.ADD_CO("tl", "tl", "S0")
    b.ADDC("th", "th", "S1")
    b.BITOP3("dl", "tl", "S0", "xl", lambda t_, vp, x: (t_ ^ vp) | x)
    b.BITOP3("dh", "th", "S1", "xh", lambda t_, vp, x: (t_ ^ vp) | x)
    b.BITOP3("hpl", "dl", "S0", "S2", lambda d, vp, vn: ~(d | vp) | vn)
    b.BITOP3("hph", "dh", "S1", "S3", lambda d, vp, vn: ~(d | vp) | vn)
    b.AND("hnl", "dl", "S0")
    b.AND("hnh", "dh", "S1")
    b.ALIGNBIT("x2l", "dh", "dl", "$one")      # (D0 >> 1) low word
    b.LSHR1("x2h", "dh")
    b.AND("S2", "x2l", "hpl")
    b.AND("S3", "x2h", "hph")
    b.BITOP3("S0", "hpl", "x2l", "hnl", lambda hp, x2, hn: ~(hp | x2) | hn)
    b.BITOP3("S1", "hph", "x2h", "hnh", lambda hp, x2, hn: ~(hp | x2) | hn)
    b.BITOP3("e", "dl", "$one", "$one", lambda d, one, _o: ~d & one)
    b.ADD("S4", "S4", "e")
    return b


BANDED_PHASE_MIN = 8   # bgsa_common.h: kBandedPhaseMin


def banded_phase_rows(k: int) -> int:
    """Rows a 32-bit word can hold the band of threshold k IN PLACE (bgsa_common.h: banded_phase_rows): the band's
    2k + 1 bits start at bit 0, move up one bit per row, and the bit above them must still exist in the phase's last
    row.  0 = no room worth using (k > 11): those thresholds run the sliding form (banded_body)."""
    rows = 31 - 2 * k
    return rows if rows >= BANDED_PHASE_MIN else 0


def banded_phase_body() -> Body:
    """The band held in place (k <= 11; BGSA_BANDED_IMPL=p, measured and NOT the default): for banded_phase_rows(k) rows
    the match window of each class is fixed (E0 = the phase's window of the row's class, one funnel shift per class
    and PHASE instead of one per row) and the band moves up one bit per row inside the register, which is the
    classical recurrence — HP and HN move left through x + x, fast class — instead of the sliding one (D0 >> 1,
    half-rate class).  Every instruction of the row is fast class, and the row alone is ≈ 7 % faster than
    banded_body's; but every phase ends with a re-anchoring event (two shifts, a popcount, five funnel shifts — all
    half-rate — plus the event's scalar path) that costs as much as 2.6 rows, so at k = 8 (15 rows per phase) the
    loop is 8 % SLOWER than the sliding form, and still 4 % slower at k = 2 (27 rows per phase).  DESIGN.md §4.4.
    State: S0 = VP, S1 = VN (at the row's offset), S2 = errors counted before this phase (since row k), S3 = the band
    mask at the row's offset, S4 = its lowest bit, S5 = the phase's error bits: ~D0 on the lowest diagonal, one bit
    per row (errors so far = S2 + popcount(S5)).  Bits outside the band hold no information: below it the masked
    match word generates no carry, above it only the first bit is read and it is the band's carry-out whatever VP
    holds there."""
    b = Body()
    b.BITOP3("x", "E0", "S1", "S3", lambda w, vn, m: (w | vn) & m)
    b.AND("t", "x", "S0")
    b.ADD("t", "t", "S0")
    b.BITOP3("d0", "t", "S0", "x", lambda t, vp, x: (t ^ vp) | x)
    b.BITOP3("hp", "d0", "S0", "S1", lambda d, vp, vn: ~(d | vp) | vn)
    b.AND("hn", "d0", "S0")
    b.ADD("hp", "hp", "hp")
    b.ADD("hn", "hn", "hn")
    b.AND("S1", "d0", "hp")
    b.BITOP3("S0", "d0", "hp", "hn", lambda d, hp, hn: ~(d | hp) | hn)
    b.BITOP3("S5", "S5", "d0", "S4", lambda a, d, sel: a | (~d & sel))
    b.ADD("S3", "S3", "S3")
    b.ADD("S4", "S4", "S4")
    return b


def banded_last_check(length: int, k: int) -> int:
    """Rows after which the reference runs its last err > max_err test (banded.hip)."""
    h = k
    return length if length <= 64 else max(64, length - h)


BANDED_CHECK_ROWS = 8   # bgsa_common.h: kBandedCheckRows
BANDED_LATE_ROWS = 48   # bgsa_common.h: kBandedLateRows


def banded_tokens(length: int, k: int, word_bits: int = 32, phase: int = 0, cut: int = 0):
    """The per-query token sequence of the banded stream, query characters as ('row', r):
    ('event', bits) with bits 1 = reset the error count (row k), 2 = advance the match-string
    words (every word_bits rows), 4 = test err > limit on all lanes, 8 = latch the reject mask
    (the reference's last checkpoint), 16 = re-anchor the band (every `phase` rows; 0, the default: the sliding
    form, no such event), 32 = cut the next one-word window (every `cut` rows that do not also advance the words;
    0: the funnel-shift row, no such event).  Mirrors banded_stream_layout() in bgsa_common.h."""
    last = banded_last_check(length, k)
    out, pending = [], 0
    for r in range(length):
        if r == k:
            pending |= 1
        if r > 0 and r % word_bits == 0:
            pending |= 2
        if phase and r > 0 and r % phase == 0:
            pending |= 16
        if cut and r > 0 and r % cut == 0 and r % word_bits != 0:
            pending |= 32
        if pending:
            out.append(("event", pending))
            pending = 0
        out.append(("row", r))
        done = r + 1
        if done > k and done <= last:
            if done == last:
                pending |= 4 | 8
            elif done % BANDED_CHECK_ROWS == 0 and done - k > k + 1 and \
                    not (done > k + BANDED_LATE_ROWS and done % (2 * BANDED_CHECK_ROWS) != 0):
                pending |= 4
    if pending:
        out.append(("event", pending))
    return out


BANDED_SINGLE, BANDED_END, BANDED_REFILL, BANDED_EVENT = 25, 30, 31, 63


def banded_stream_bytes(length: int, k: int, codes, phase: int = 0, cut: int = 0) -> list:
    """The packed banded stream, byte for byte as bgsa_common.h: banded_stream_layout() writes it:
    banded_tokens() with two consecutive rows folded into one token (5*a + b) wherever no event sits
    between them, one-row tokens 25 + c otherwise, EVENT = {63, bits}, 7 payload bytes + REFILL per
    8-byte window, a two-byte token never split across windows, END padding and one spare END window."""
    out, slot = [], 0

    def put(b):
        nonlocal slot
        out.append(b)
        slot += 1
        if slot == 7:
            out.append(BANDED_REFILL)
            slot = 0

    def put_event(bits):
        nonlocal slot
        if slot == 6:
            out.extend([BANDED_REFILL, BANDED_END])
            slot = 0
        put(BANDED_EVENT)
        put(bits)

    toks = banded_tokens(length, k, phase=phase, cut=cut)
    i = 0
    while i < len(toks):
        kind, val = toks[i]
        if kind == "event":
            put_event(val)
            i += 1
        elif i + 1 < len(toks) and toks[i + 1][0] == "row":
            put(5 * int(codes[val]) + int(codes[toks[i + 1][1]]))
            i += 2
        else:
            put(BANDED_SINGLE + int(codes[val]))
            i += 1
    put(BANDED_END)
    while len(out) % 8:
        out.append(BANDED_END)
    out.extend([BANDED_END] * 8)
    return out


def banded_simulate(subjects: np.ndarray, query: np.ndarray, k: int, wide: bool | None = None,
                    phase: int = 0, cut: int = 0, groups: int = 1) -> np.ndarray:
    """Whole banded pipeline on the CPU with the shipped row body: Mext preprocess, token stream, events, final band walk.
    Returns int8 results like the kernel; 127 for a lane over the limit at the latching test, and for every lane once a test
    finds all of them over (the kernels stop there).  Four forms share the loop; the first that applies runs:
      wide (the default for k > 15): banded_body64 on register pairs, three match-string words per row;
      phase = banded_phase_rows(k): banded_phase_body as banded_asm_kernel<false, true> runs it — the prologue's window is the
        first match word with the mask at offset 0, a re-anchor event every `phase` rows, the epilogue shifts by the rows of
        the last phase and folds the collected error bits;
      cut = banded_cut_rows(k): banded_cut_body(groups) as banded_cut_kernel<G> runs it — the subjects split into `groups`
        parts that share the token stream, and per class two registers: A, the window the row shifts by the rows since the
        last cut, and B, the next word (advance: A <- B, B <- the next word; cut: A <- {B >> bits cut so far, A} >> cut);
      otherwise banded_body, two match-string words per row."""
    if wide is None:
        wide = k > 15
    phase = 0 if wide else phase
    cut = 0 if wide or phase else cut
    groups = groups if cut else 1
    n, length = subjects.shape
    assert n % groups == 0
    per = n // groups
    sl = [slice(g * per, (g + 1) * per) for g in range(groups)]
    mext = build_peq32(subjects, (length + 31) // 32 + (3 if wide or cut else 2), offset=k + 1)
    band = (1 << (2 * k + 1)) - 1
    z = lambda: np.zeros(per, dtype=np.uint32)
    body = banded_body64() if wide else banded_phase_body() if phase else banded_cut_body(groups) if cut else banded_body()
    n_state = 5 if wide else 6 if phase else 3
    st = [z() for _ in range(n_state * groups)]
    if phase:
        st[3], st[4] = np.full(n, band, np.uint32), np.ones(n, np.uint32)
        win = [mext[c, 0].copy() for c in range(5)]
    if cut:
        A = [[mext[c, 0, s].copy() for c in range(5)] for s in sl]      # row 0: the first word itself
        B = [[mext[c, 1, s].copy() for c in range(5)] for s in sl]
    ERR = 4 if wide else 2

    def errors(g):      # counted on the lowest diagonal since row k
        return st[n_state * g + ERR] + (np.bitwise_count(st[5]).astype(np.uint32) if phase else np.uint32(0))

    def alignbit(hi, lo, s):
        return ((((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(s)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)

    dead = np.zeros(n, dtype=bool)
    wi = sh = off = in_phase = 0
    qcode = CLASS_CODE[query]
    for kind, val in banded_tokens(length, k, phase=phase, cut=cut):
        if kind == "row":
            c = int(qcode[val])
            assert not cut or (sh < cut and sh + 2 * k + 1 <= 32)
            eq = [win[c]] if phase else [A[g][c] for g in range(groups)] if cut else [mext[c, wi + i] for i in range(3 if wide else 2)]
            body.simulate(st, eq, scalars={"$sh": sh, "$mask": band & 0xFFFFFFFF, "$mask_lo": band & 0xFFFFFFFF,
                                           "$mask_hi": band >> 32, "$one": 1})
            sh += 1
            in_phase += 1
            continue
        if val & 4:      # test err > limit on all lanes
            over = np.concatenate([errors(g) > np.uint32(k + 1) for g in range(groups)])
            if val & 8:  # the reference's last checkpoint: latch the reject mask
                dead = over.copy()
            if over.all():
                return np.full(n, 127, dtype=np.int8)
        if val & 1:      # row k: the count starts
            for g in range(groups):
                st[n_state * g + ERR] = z()
            if phase:
                st[5] = z()
        if val & 2:      # advance the match-string words
            wi, sh, off = wi + 1, 0, 0
            for g in range(groups if cut else 0):
                A[g], B[g] = B[g], [mext[c, wi + 1, sl[g]].copy() for c in range(5)]
        if val & 16:     # re-anchor the band
            assert in_phase == phase
            st[0], st[1], st[2] = st[0] >> np.uint32(phase), st[1] >> np.uint32(phase), errors(0)
            st[3], st[4], st[5] = np.full(n, band, np.uint32), np.ones(n, np.uint32), z()
            win = [alignbit(mext[c, wi + 1], mext[c, wi], sh) for c in range(5)]
            in_phase = 0
        if val & 32:     # cut the next one-word window
            for g in range(groups):
                A[g] = [alignbit(B[g][c] >> np.uint32(off), A[g][c], cut) for c in range(5)]
            off, sh = off + cut, 0
            for g in range(groups):      # what the window must be: bits off.. of the 64-bit pair of this advance
                for c in range(5):
                    assert np.array_equal(A[g][c], alignbit(mext[c, wi + 1, sl[g]], mext[c, wi, sl[g]], off))
    if phase:
        assert in_phase == length - phase * ((length - 1) // phase)
    out = np.empty(n, dtype=np.int8)
    for g in range(groups):
        S = [x.astype(np.uint64) for x in st[n_state * g:n_state * (g + 1)]]
        if wide:
            vp, vn = S[0] | (S[1] << np.uint64(32)), S[2] | (S[3] << np.uint64(32))
        else:            # the phase form's band sits in_phase bits up
            vp, vn = S[0] >> np.uint64(in_phase if phase else 0), S[1] >> np.uint64(in_phase if phase else 0)
        err = errors(g).astype(np.int64) + k
        best = err.copy()
        for i in range(k + 1):
            err = err + ((vp >> np.uint64(i)) & np.uint64(1)).astype(np.int64) - ((vn >> np.uint64(i)) & np.uint64(1)).astype(np.int64)
            best = np.minimum(best, err)
        out[sl[g]] = np.where(dead[sl[g]], 127, best).astype(np.int8)
    return out


# =================================================================================================
# BitPAl packed for any integer scores (match M > mismatch I >= 2*gap G, G < 0): the scheme the
# reference's generator emits per score set (generator/.../BitPAlGenerator.java:151-534 packed form,
# ScoreMsg.java:23-31 for the value ranges), restated on normalised differences.
#
#   u_j = dH(row above, column j) - G   in [0, C],  C = M - 2G      (stored unsigned on bits(C) planes)
#   v_j = dV(column j)            - G   in [0, C]
#   v_j = max(0, w_j - u_j),  w_j = C at a match, else max(D, v_{j-1}),  D = I - 2G
#   new u_j = max(0, max(W_j, u_j) - v_{j-1}),  W_j = C at a match, D otherwise
#
# Only the K = M - I values above D survive a mismatch unchanged, so the row resolves the chain
# v_{j-1} -> v_j per value class C, C-1, ..., D+1 with one add-with-carry run propagation each (the
# value is kept across columns with u = 0) and treats everything else as class D.
# =================================================================================================

@dataclass(frozen=True)
class BitpalScores:
    match: int = 2
    mismatch: int = -3
    gap: int = -5

    def __post_init__(self):
        if not (self.match > self.mismatch and self.mismatch >= 2 * self.gap and self.gap < 0):
            raise ValueError("BitPAl needs match > mismatch >= 2*gap and gap < 0")

    @property
    def C(self) -> int: return self.match - 2 * self.gap          # largest normalised difference
    @property
    def D(self) -> int: return self.mismatch - 2 * self.gap       # the mismatch class
    @property
    def K(self) -> int: return self.match - self.mismatch         # value classes above D
    @property
    def nb(self) -> int: return self.C.bit_length()               # magnitude planes
    @property
    def planes(self) -> int: return self.nb                       # unsigned u: no sign plane
    @property
    def chains(self) -> int: return 1 + (1 if BITPAL_ONE_CHAIN else 2) * (self.K - 1) + self.nb
    @property
    def tag(self) -> str:
        f = lambda v: f"m{-v}" if v < 0 else f"{v}"
        return f"{f(self.match)}_{f(self.mismatch)}_{f(self.gap)}"

    def weights(self) -> tuple:
        """Per-plane weight of a set bit in the final score: u = sum 2^i p_i."""
        return tuple(1 << i for i in range(self.nb))


BITPAL_DEFAULT = BitpalScores(2, -3, -5)
BITPAL_SCHEDULE_WINDOW = int(_knob('BITPAL_WINDOW', '48'))   # 0 = program order (A/B)
# build-time A/B switches of round 4's two rewrites of the row body (see _bitpal_scores_body; scripts/r04_bitpal_ab.sh,
# profiles/r04_bitpal_ab.txt, 10k x 1M x 150 bp on one box): reading "u <= D" off its plane — one instruction fewer — measured
# 6,893 -> 6,854 ms and is on; one addition chain per class instead of two — same count, 13 -> 9 chains — measured 6,893 -> 6,949 ms
# (and the chip held a lower clock under it) and is OFF
BITPAL_ONE_CHAIN = _knob('BITPAL_ONE_CHAIN', '0') != '0'
BITPAL_INLINE_LE = _knob('BITPAL_INLINE_LE', '1') != '0'
# round 4, second step: new u = max(w, u) - v_in needs no clamp (see _bitpal_scores_body: "the cell identity"); '0' builds the
# previous form, new u = max(0, max(W, u) - v_in), for A/B
BITPAL_CELL_MAX = _knob('BITPAL_CELL_MAX', '1') != '0'
# the one-hot mask of u = K - 1 has ONE reader — the lowest class's seed term with the top class — so that product is formed from the
# planes and the class mask directly: one instruction per word fewer ('0': the mask is built like the others, for A/B)
BITPAL_FOLD_LAST_Z = _knob('BITPAL_FOLD_LAST_Z', '1') != '0'
# the run mask (u = 0 at a MISMATCH) is not needed: the classes may propagate through every u = 0 column — what runs through a u = 0
# match column is covered, column by column, by the top class's own propagation from that very column, and the extraction masks
# with the top class instead of the match mask.  One instruction per word fewer ('0': the run mask, for A/B).
BITPAL_NO_RUN = _knob('BITPAL_NO_RUN', '1') != '0'



class _Bool:
    """Boolean-expression helper over a Body with common-subexpression sharing per word."""

    def __init__(self, body: Body, prefix: str):
        self.b = body
        self.memo = {}
        self.n = 0
        self.prefix = prefix

    def _name(self, hint):
        self.n += 1
        return f"{hint}{self.prefix}_{self.n}"

    def op3(self, fn, a, b_, c, hint="x"):
        # canonical operand order, so that e.g. OR3(p0, p1, p2) and OR3(p2, p1, p0) are one instruction
        order = sorted(range(3), key=lambda i: (a, b_, c)[i])
        ops = [(a, b_, c)[i] for i in order]

        def g(x0, x1, x2, order=order, fn=fn):
            args = [None, None, None]
            for pos, i in enumerate(order):
                args[i] = (x0, x1, x2)[pos]
            return fn(*args)

        key = (tt(g), *ops)
        if key not in self.memo:
            self.memo[key] = self.b.BITOP3(self._name(hint), ops[0], ops[1], ops[2], g)
        return self.memo[key]

    def op2(self, kind, a, b_, hint="x"):
        key = (kind, a, b_)
        if key not in self.memo:
            self.memo[key] = getattr(self.b, kind)(self._name(hint), a, b_)
        return self.memo[key]

    def or_all(self, names, hint="o"):
        names = list(names)
        while len(names) > 1:
            if len(names) == 2:
                return self.op2("OR", names[0], names[1], hint)
            merged = self.op3(lambda a, b_, c: a | b_ | c, names[0], names[1], names[2], hint)
            names = [merged] + names[3:]
        return names[0]

    def and_pattern(self, planes, bits, hint="z"):
        """AND over planes of (plane if bit else ~plane); planes given MSB first.  Chunks are taken
        from the MSB side so that patterns sharing their high bits share the partial products."""
        n = len(planes)
        lit = lambda x, bit: x if bit else ~x
        first = 3 if n >= 3 and (n - 3) % 2 == 0 else 2
        if first == 3:
            b0, b1, b2 = bits[:3]
            cur = self.op3(lambda a, b_, c: lit(a, b0) & lit(b_, b1) & lit(c, b2), planes[0], planes[1], planes[2], hint)
        else:
            b0, b1 = bits[:2]
            cur = self.op3(lambda a, b_, c: lit(a, b0) & lit(b_, b1), planes[0], planes[1], planes[1], hint)
        i = first
        while i < n:
            b0, b1 = bits[i], bits[i + 1]
            cur = self.op3(lambda a, b_, c: a & lit(b_, b0) & lit(c, b1), cur, planes[i], planes[i + 1], hint)
            i += 2
        return cur


@functools.lru_cache(maxsize=256)
def bitpal_body(nw: int, sc: BitpalScores = BITPAL_DEFAULT) -> Body:
    """For the default scores this computes what the packed kernel of original/BGSA_AVX2/align_core.c:
    183-428 computes (194 ALU operations per word there), on four unsigned planes, in 69 fast-class VALU.
    (Memoised: callers treat the returned Body as read-only.)  The row body for `nw` words, with the single-use one-hot mask folded into
    its seed product where that saves an instruction for this score set (it does when the mask shares no partial product with the others:
    2/-3/-5 64 -> 63; 10/-9/-15 would lose one)."""
    if BITPAL_FOLD_LAST_Z and _bitpal_scores_body(1, sc, True).valu_count() < _bitpal_scores_body(1, sc, False).valu_count():
        return _bitpal_scores_body(nw, sc, True)
    return _bitpal_scores_body(nw, sc, False)


@__import__("functools").lru_cache(maxsize=512)
def _bitpal_scores_body(nw: int, sc: BitpalScores, fold_last_z: bool) -> Body:
    """Row body for `nw` words.  State S[w*B + i] = plane i (weight 2^i) of the UNSIGNED value u of word
    w's 32 columns, B = sc.planes = bits(C) (the reference keeps the two's complement of -u in one more
    plane, align_core.c:191-214; the unsigned form saves that plane and four instructions per word).
    E[w] = match mask.  Chains (in order): the top-class run, then per lower class the seed shift and its run (one chain
    for both under BGSA_GEN_BITPAL_ONE_CHAIN=1, measured slower), then the B plane shifts — sc.chains in all."""
    B, C, D, K = sc.planes, sc.C, sc.D, sc.K
    b = Body()
    U = lambda w, i: f"S{w * B + i}"
    E = lambda w: f"E{w}"
    t = lambda name, w: f"{name}_{w}"
    W = range(nw)
    z = {}      # (value of u, word) -> one-hot mask name
    anym = {}   # word -> mismatch columns whose u <= D
    le_plane = {}   # word -> the ONE plane p with "u <= D  <=>  ~p" (D + 1 a power of two): no mask of its own is built
    dv = {}     # (class offset c, word) -> columns whose incoming v is C - c (c = 0: or a match)
    prop, stop = {}, {}   # word -> the columns a class value runs through unchanged; the columns that end up in the top class whatever arrives

    # ---- decode the u classes the seeds need, the "u <= D" mask, and the top-class run ----------
    for w in W:
        bx = _Bool(b, f"d{w}")
        planes = [U(w, i) for i in range(B)]
        msb_first = planes[::-1]
        if B == 1:
            z0 = bx.op3(lambda a, _a, __a: ~a, planes[0], planes[0], planes[0], "z0")
        elif B == 2:
            z0 = bx.op3(lambda a, b_, _b: ~(a | b_), planes[0], planes[1], planes[1], "z0")
        elif K > 1 and B > 3:
            # u == 0 shares the "high planes are zero" product with the small-u masks below
            z0 = bx.and_pattern(msb_first, [0] * B, "z")
        else:
            low = bx.or_all(planes[:B - 2], "lo") if B > 3 else planes[0]
            z0 = bx.op3(lambda a, b_, c: ~(a | b_ | c), low, planes[B - 2], planes[B - 1], "z0")   # u == 0
        for x in range(1, K):
            if fold_last_z and x == K - 1 and K > 2 and B > 1:
                continue      # read once, by seed K-1's first term: folded into that product below
            z[x, w] = bx.and_pattern(msb_first, [(x >> i) & 1 for i in range(B - 1, -1, -1)]) if B > 1 else planes[0]
        # u <= D: constant comparator from the LSB up (r = "the bits seen so far are <= the constant's";
        # a one bit of D ORs the complemented plane in, a zero bit ANDs it)
        step = lambda rv, p, bit: (~p | rv) if bit else (~p & rv)
        i = 0
        while i < B and (D >> i) & 1:      # trailing one bits of the constant: always satisfied
            i += 1
        if BITPAL_CELL_MAX:
            pass                               # max_planes() takes max(w, u) from the first subtract's borrow: nobody reads "u <= D"
        elif i >= B:
            anym[w] = bx.op3(lambda e, _e, __e: ~e, E(w), E(w), E(w), "any")          # every u is <= D
        else:
            r = None
            first = i
            i += 1
            # the first zero bit: r = ~plane
            pending = [("not", planes[first])]
            cur = None
            while i < B:
                b0 = (D >> i) & 1
                if i + 1 < B:
                    b1 = (D >> (i + 1)) & 1
                    if cur is None:
                        cur = bx.op3(lambda x1, x0, p, b0=b0, b1=b1: step(step(~p, x0, b0), x1, b1),
                                     planes[i + 1], planes[i], planes[first], "le")
                    else:
                        cur = bx.op3(lambda x1, x0, rv, b0=b0, b1=b1: step(step(rv, x0, b0), x1, b1),
                                     planes[i + 1], planes[i], cur, "le")
                    i += 2
                else:
                    if cur is None:
                        cur = bx.op3(lambda x0, p, _p, b0=b0: step(~p, x0, b0), planes[i], planes[first], planes[first], "le")
                    else:
                        cur = bx.op3(lambda x0, rv, _r, b0=b0: step(rv, x0, b0), planes[i], cur, cur, "le")
                    i += 1
            if cur is None and BITPAL_INLINE_LE:   # the comparison is just "~plane[first]": max_planes() reads that plane itself
                le_plane[w] = planes[first]
            elif cur is None:
                anym[w] = bx.op3(lambda p, e, _e: ~p & ~e, planes[first], E(w), E(w), "any")
            else:
                anym[w] = bx.op3(lambda le, e, _e: le & ~e, cur, E(w), E(w), "any")
        b.AND(t("seed", w), z0, E(w))
        if BITPAL_NO_RUN:
            prop[w] = z0
            (b.ADD_CO if w == 0 else b.ADDC)(t("sum", w), t("seed", w), z0)
            dv[0, w] = b.BITOP3(t("dvtop", w), t("sum", w), z0, E(w), lambda s, z_, e: (s ^ (z_ & ~e)) | e)
            stop[w] = dv[0, w]
            continue
        b.XOR(t("run", w), z0, t("seed", w))                       # u == 0 at a mismatch
        prop[w], stop[w] = t("run", w), E(w)
        (b.ADD_CO if w == 0 else b.ADDC)(t("sum", w), t("seed", w), z0)
        dv[0, w] = b.BITOP3(t("dvtop", w), t("sum", w), t("run", w), E(w), lambda s, r, e: (s ^ r) | e)

    def shifted_run(seed_name, c):
        # The seeds act one column up and spread over the run behind them: (seed << 1) + run.  A seed sits on a column with
        # u > 0, a run column has u = 0, so the two are disjoint and (seed << 1) + run = seed + (seed | run): ONE addition
        # with carry across the words instead of a shift chain and an addition chain (13 -> 9 chains for 2/-3/-5, same
        # instruction count).  Built, bit-exact, measured 0.8 % SLOWER on the full config 4: the A/B alternative.
        if not BITPAL_ONE_CHAIN:      # round 3's form: a shift chain, then an addition chain
            for w in W:
                (b.ADD_CO if w == 0 else b.ADDC)(t(seed_name, w), t(seed_name, w), t(seed_name, w))
            for w in W:
                (b.ADD_CO if w == 0 else b.ADDC)(t(f"rs{c}", w), t(seed_name, w), prop[w])
                dv[c, w] = b.BITOP3(t(f"dv{c}", w), t(f"rs{c}", w), prop[w], stop[w], lambda s, r, e: (s ^ r) & ~e)
            return
        for w in W:
            b.OR(t(f"sr{c}", w), t(seed_name, w), prop[w])
        for w in W:
            (b.ADD_CO if w == 0 else b.ADDC)(t(f"rs{c}", w), t(f"sr{c}", w), t(seed_name, w))
            dv[c, w] = b.BITOP3(t(f"dv{c}", w), t(f"rs{c}", w), prop[w], stop[w], lambda s, r, e: (s ^ r) & ~e)

    # ---- classes C-1 .. D+1: value C-c appears where an incoming class C-x meets u = c-x ----------
    for c in range(1, K):
        for w in W:
            if (c, w) not in z:      # fold_last_z: [u = K - 1] AND the top class in one product over the planes and the mask
                msb_first = [U(w, i) for i in range(B)][::-1]
                _Bool(b, f"q{w}").and_pattern(msb_first + [dv[0, w]], [(c >> i) & 1 for i in range(B - 1, -1, -1)] + [1], "zs")
                b.ops[-1].dst = t(f"seed{c}", w)      # the product's last instruction IS the seed's first term: name it so
            else:
                b.AND(t(f"seed{c}", w), z[c, w], dv[0, w])
            for x in range(1, c):
                b.BITOP3(t(f"seed{c}", w), z[c - x, w], dv[x, w], t(f"seed{c}", w), lambda a, b_, acc: (a & b_) | acc)
        shifted_run(f"seed{c}", c)

    # ---- w planes, v = max(0, w - u) = (w + ~u + 1) where that does not borrow, else 0 ------------------
    lit = {"reg": lambda x: x, "not": lambda x: ~x, "zero": lambda x: 0, "one": lambda x: 0xFF}

    def subtract(w, minuend, sub_name, out_name, top_out=None, clamp=True, out_reg=None):
        """out = max(0, minuend - sub) over B planes; minuend[i] = (kind, register name or None).  The top plane
        comes out clamped (into `top_out` if given); the caller ANDs planes 0..B-2 with the returned mask.
        clamp = False: the caller knows minuend >= sub — plain difference, plane i into out_reg(i), no borrow out of the top plane."""
        carry = None
        dst = (lambda i: out_reg(i)) if out_reg is not None else (lambda i: t(f"{out_name}{i}", w))
        for i in range(B):
            kind, name = minuend[i]
            f = lit[kind]
            src = name if name is not None else sub_name(i)
            if carry is None:      # bit 0: the +1 of the two's complement is the carry-in
                if kind == "reg":
                    b.XOR(dst(i), src, sub_name(i))
                else:
                    b.BITOP3(dst(i), src, sub_name(i), sub_name(i), lambda m, s, _s, f=f: f(m) ^ s)
                if B > 1 or clamp:
                    carry = b.BITOP3(t(f"{out_name}c", w), src, sub_name(i), sub_name(i), lambda m, s, _s, f=f: f(m) | ~s)
            elif i == B - 1 and not clamp:
                b.BITOP3(dst(i), src, sub_name(i), carry, lambda m, s, cy, f=f: f(m) ^ ~s ^ cy)
                carry = None
            elif i == B - 1:
                # top plane: its clamp (difference bit AND "no borrow out of this plane") is a function of the same three
                # inputs, so it costs no instruction of its own
                maj = lambda m, s, cy, f=f: (f(m) & ~s) | (f(m) & cy) | (~s & cy)
                prev = carry
                carry = b.BITOP3(t(f"{out_name}c{i}", w), src, sub_name(i), prev, maj)
                b.BITOP3(top_out or t(f"{out_name}{i}", w), src, sub_name(i), prev,
                         lambda m, s, cy, f=f, maj=maj: (f(m) ^ ~s ^ cy) & maj(m, s, cy))
            else:
                b.BITOP3(dst(i), src, sub_name(i), carry, lambda m, s, cy, f=f: f(m) ^ ~s ^ cy)
                carry = b.BITOP3(t(f"{out_name}c", w), src, sub_name(i), carry,
                                 lambda m, s, cy, f=f: (f(m) & ~s) | (f(m) & cy) | (~s & cy))
        return carry     # 1 = no borrow: the difference is >= 0; planes 0..B-2 still need their AND with it

    w_of, ok_of = {}, {}    # word -> the planes of w as subtract() takes them; the "w >= u" mask of the first subtract
    for w in W:
        bx = _Bool(b, f"w{w}")
        cls_mask = {C - c: dv[c, w] for c in range(K)}
        # plane i of w over the columns: classes above D contribute their masks, class D is "the rest".
        # Either spell every plane from the class masks alone, or spend the ops for rest = ~OR(all masks)
        # once and use it as one more mask — whichever costs fewer instructions overall.
        or_cost = lambda n: 0 if n <= 1 else n // 2
        have = [[v for v in cls_mask if (v >> i) & 1] for i in range(B)]
        lack = [[v for v in cls_mask if not (v >> i) & 1] for i in range(B)]
        d_bit = [(D >> i) & 1 for i in range(B)]

        def plan(with_rest):
            total, choice = (or_cost(K) if with_rest else 0), []
            for i in range(B):
                opts = []
                if with_rest:   # rest joins the side class D is on
                    opts.append((or_cost(len(have[i]) + d_bit[i]), "reg", have[i], bool(d_bit[i])))
                    opts.append((or_cost(len(lack[i]) + 1 - d_bit[i]), "not", lack[i], not d_bit[i]))
                elif d_bit[i]:
                    opts.append((or_cost(len(lack[i])), "not", lack[i], False))
                else:
                    opts.append((or_cost(len(have[i])), "reg", have[i], False))
                best = min(opts, key=lambda o: o[0])
                total += best[0]
                choice.append(best)
            return total, choice

        (cost_r, choice_r), (cost_n, choice_n) = plan(True), plan(False)
        use_rest = cost_r < cost_n
        rest = None
        if use_rest:
            allm = [cls_mask[v] for v in cls_mask]
            if len(allm) == 1:
                rest = bx.op3(lambda a, _a, __a: ~a, allm[0], allm[0], allm[0], "rest")
            elif len(allm) == 2:
                rest = bx.op3(lambda a, b_, _b: ~(a | b_), allm[0], allm[1], allm[1], "rest")
            else:
                head = bx.or_all(allm[:-2], "hi") if len(allm) > 3 else allm[0]
                rest = bx.op3(lambda a, b_, c: ~(a | b_ | c), head, allm[-2], allm[-1], "rest")
        wplanes = []   # (kind, name): plane i of w is name / ~name / 0 / 1
        for _cost, kind, vals, plus_rest in (choice_r if use_rest else choice_n):
            masks = [cls_mask[v] for v in vals] + ([rest] if plus_rest else [])
            if not masks:
                wplanes.append(("zero" if kind == "reg" else "one", None))
            else:
                wplanes.append((kind, bx.or_all(masks, "wp")))
        ok = subtract(w, wplanes, lambda i, w=w: U(w, i), "s")
        w_of[w], ok_of[w] = wplanes, ok
        for i in range(B - 1 if B > 1 else B):
            b.AND(t(f"s{i}", w), t(f"s{i}", w), ok)

    # ---- max(W, u): C at a match, D at a mismatch with u <= D, else u -------------------------------
    def max_planes(w):
        if BITPAL_CELL_MAX:
            # The cell identity: with a = u, b = v_in and W the cell's substitution value, v = max(0, max(W, b) - a) and
            # new u = max(0, max(W, a) - b) are m - a and m - b for m = max(W, a, b) — the largest of the three can be clamped by
            # neither.  w = max(W, b) is in hand (the class masks), "w >= u" is the first subtract's borrow: m = w or u by that
            # mask, one instruction per plane (what max(W, u) cost), and the second subtract needs no clamp and no borrow out of
            # its top plane: four instructions per word fewer (2/-3/-5: 68 -> 64), and the "u <= D" comparator has no reader left.
            for i in range(B):
                kind, name = w_of[w][i]
                f = lit[kind]
                if name is None:
                    b.BITOP3(t(f"g{i}", w), U(w, i), ok_of[w], ok_of[w], lambda u, ok, _ok, f=f: (f(0) & ok) | (u & ~ok))
                else:
                    b.BITOP3(t(f"g{i}", w), name, U(w, i), ok_of[w], lambda wp, u, ok, f=f: (f(wp) & ok) | (u & ~ok))
            return
        for i in range(B):
            cb, db = 0xFF * ((C >> i) & 1), 0xFF * ((D >> i) & 1)
            if w in le_plane:      # "u <= D" is the complement of one plane: read it directly (one instruction per word saved)
                p = le_plane[w]
                if U(w, i) == p:
                    b.BITOP3(t(f"g{i}", w), p, p, E(w), lambda u, _u, e, cb=cb, db=db: (cb & e) | (db & ~u & ~e) | (u & ~e))
                else:
                    b.BITOP3(t(f"g{i}", w), U(w, i), p, E(w),
                             lambda u, p_, e, cb=cb, db=db: (cb & e) | (db & ~p_ & ~e) | (u & p_ & ~e))
                continue
            b.BITOP3(t(f"g{i}", w), U(w, i), anym[w], E(w),
                     lambda u, a, e, cb=cb, db=db: (cb & e) | (db & a & ~e) | (u & ~a & ~e))

    # ---- v one column up: B shift chains, the max-plane work interleaved into the first ---------------
    for i in range(B):
        for w in W:
            (b.ADD_CO if w == 0 else b.ADDC)(t(f"s{i}", w), t(f"s{i}", w), t(f"s{i}", w))
            if i == 0:
                max_planes(w)

    # ---- new u = max(0, max(W, u) - v_in) -------------------------------------------------------------
    for w in W:
        if BITPAL_CELL_MAX:
            subtract(w, [("reg", t(f"g{i}", w)) for i in range(B)], lambda i, w=w: t(f"s{i}", w), "r", clamp=False,
                     out_reg=lambda i, w=w: U(w, i))
            continue
        ok = subtract(w, [("reg", t(f"g{i}", w)) for i in range(B)], lambda i, w=w: t(f"s{i}", w), "r",
                      top_out=U(w, B - 1) if B > 1 else None)
        for i in range(B - 1 if B > 1 else B):
            b.AND(U(w, i), t(f"r{i}", w), ok)
    # chains first, their wait states filled with independent work (no extra registers)
    return schedule(b, BITPAL_SCHEDULE_WINDOW) if BITPAL_SCHEDULE_WINDOW else b


def bitpal_init_state(nw: int, lanes: int, sc: BitpalScores = BITPAL_DEFAULT, semi: bool = False) -> list:
    """Row 0: every column at dH = G (global), or at dH = 0, i.e. u = -G (semi-global: the
    generator's writeBitInitStr, BitPAlGenerator.java:2201-2218)."""
    stored = -sc.gap if semi else 0                                   # u itself
    return [np.full(lanes, 0xFFFFFFFF if (stored >> i) & 1 else 0, dtype=np.uint32)
            for _ in range(nw) for i in range(sc.planes)]


def bitpal_column_values(state: list, w: int, sc: BitpalScores) -> np.ndarray:
    """u of the 32 columns of word w: [lanes, 32] int64."""
    B = sc.planes
    bits = np.arange(32, dtype=np.uint32)
    u = np.zeros((state[0].shape[0], 32), dtype=np.int64)
    for i, wt in enumerate(sc.weights()):
        u += wt * ((state[w * B + i][:, None] >> bits[None, :]) & np.uint32(1)).astype(np.int64)
    return u


def bitpal_score(state: list, nw: int, qlen: int, slen: int, sc: BitpalScores = BITPAL_DEFAULT,
                 semi: bool = False) -> np.ndarray:
    """Global: S[m][n] = G*(m + n) + sum over subject columns of u.  Semi-global: the maximum of
    S[m][j] = G*m + sum_{c <= j} (u_c + G) over j = 0..n (genPackedScore, BitPAlGenerator.java:78-116)."""
    B = sc.planes
    if semi:
        u = np.concatenate([bitpal_column_values(state, w, sc) for w in range(nw)], axis=1)[:, :slen]
        run = sc.gap * qlen + np.cumsum(u + sc.gap, axis=1)
        best = np.maximum(run.max(axis=1, initial=-(1 << 40)), sc.gap * qlen)
        return best.astype(np.int16)
    score = np.full(state[0].shape, sc.gap * (qlen + slen), dtype=np.int64)
    for w in range(nw):
        for i, wt in enumerate(sc.weights()):
            score += wt * np.bitwise_count(state[w * B + i] & _low_mask(slen - 32 * w)).astype(np.int64)
    return score.astype(np.int16)


def make_blocked(body: Body, n_state: int, n_slots: int | None = None):
    """Column-block form of a row body: every carry chain enters and leaves through a carry word
    (32 rows per word, first row in bit 31).  Chain k reads its carry-in with `x + x` on state
    register S[n_state + k] (VCC = next row's bit) and appends its carry-out with `x + x + vcc` on
    S[n_state + n_chains + k].  Returns (new body, initial carry-in bit per chain): a chain that
    started with SETC1 has carry-in 1 in the first block, the others 0.
    (myers_block_body and myers_peq_block_body are this transformation of myers_planes_body and myers_body.)"""
    chains = []          # (index of the chain's first op, initial carry)
    for i, op in enumerate(body.ops):
        if op.kind == "add_co":
            chains.append((i, 0))
        elif op.kind == "setc1":
            chains.append((i, 1))
    n = len(chains) if n_slots is None else n_slots      # n_slots: the kernel's carry-word pairs when it has more than the body has chains
    assert len(chains) <= n
    starts = {i: k for k, (i, _) in enumerate(chains)}
    out = Body()
    open_chain = None
    for i, op in enumerate(body.ops):
        if i in starts:
            if open_chain is not None:
                out.ADDC(f"S{n_state + n + open_chain}", f"S{n_state + n + open_chain}", f"S{n_state + n + open_chain}")
            k = starts[i]
            cin = f"S{n_state + k}"
            out.ADD_CO(cin, cin, cin)
            open_chain = k
            if op.kind == "add_co":
                out.ops.append(Op("addc", op.dst, op.srcs, 0))
            continue  # setc1 itself is dropped: the carry-in word supplies the 1
        out.ops.append(op)
    if open_chain is not None:
        out.ADDC(f"S{n_state + n + open_chain}", f"S{n_state + n + open_chain}", f"S{n_state + n + open_chain}")
    return out, [c for _, c in chains]


def make_blocked_packed(body: Body, n_state: int):
    """Column-block form for bodies with MANY carry chains: the carries of one row travel as bits of a few words —
    chain k in word k // 32, first chain in bit 31 — instead of one word per chain and 32 rows (make_blocked), which
    costs two registers per chain: 86 for the 43 chains of 10/-9/-15, more than a column-block kernel can hold.
    Here the block holds ceil(chains / 32) carry-in words and as many carry-out words whatever the score set:
    chain k takes its carry-in with `x + x` on S[n_state + k // 32] (VCC = the word's top bit) and appends its
    carry-out with `x + x + vcc` on S[n_state + W + k // 32]; a last, partly filled word is moved up at the end of the
    row so that its first chain sits in bit 31 again.  The words are exchanged with the neighbouring blocks EVERY
    row (the row loop loads the next row's words while it computes this one's and stores its own behind the body):
    two or three loads and stores per row against hundreds of vector instructions.  Returns (body, initial carry-in
    bit per chain, words)."""
    chains = []
    for i, op in enumerate(body.ops):
        if op.kind == "add_co":
            chains.append((i, 0))
        elif op.kind == "setc1":
            chains.append((i, 1))
    n = len(chains)
    n_words = (n + 31) // 32
    starts = {i: k for k, (i, _) in enumerate(chains)}
    cin = lambda k: f"S{n_state + k // 32}"
    cout = lambda k: f"S{n_state + n_words + k // 32}"
    out = Body()
    open_chain = None
    for i, op in enumerate(body.ops):
        if i in starts:
            if open_chain is not None:
                out.ADDC(cout(open_chain), cout(open_chain), cout(open_chain))
            k = starts[i]
            out.ADD_CO(cin(k), cin(k), cin(k))
            open_chain = k
            if op.kind == "add_co":
                out.ops.append(Op("addc", op.dst, op.srcs, 0))
            continue
        out.ops.append(op)
    if open_chain is not None:
        out.ADDC(cout(open_chain), cout(open_chain), cout(open_chain))
    if n % 32:
        last = f"S{n_state + 2 * n_words - 1}"
        out.LSHL_IMM(last, last, 32 - n % 32)
    return out, [c for _, c in chains], n_words


def bitpal_packed_block_body(nw: int, sc: BitpalScores = BITPAL_DEFAULT):
    """Packed-carry column-block form of bitpal_body: (body, initial carry-in per chain, carry words per direction)."""
    body, init, n_words = make_blocked_packed(bitpal_body(nw, sc), sc.planes * nw)
    return schedule(body, 200), init, n_words


def bitpal_packed_blocked_simulate(subjects: np.ndarray, query: np.ndarray, nw_block: int,
                                   sc: BitpalScores = BITPAL_DEFAULT, semi: bool = False) -> np.ndarray:
    """bitpal_packed_blocked_kernel at toy scale: column blocks of nw_block words, per query row the carry words of
    the block to the left are this block's carry-in words and its own carry-out words replace them."""
    n, slen = subjects.shape
    qlen = len(query)
    B = sc.planes
    nw_total = (slen + 31) // 32
    n_blocks = (nw_total + nw_block - 1) // nw_block
    peq = build_peq32(subjects, n_blocks * nw_block)
    body, init, n_words = bitpal_packed_block_body(nw_block, sc)
    assert not any(init) and n_words == (sc.chains + 31) // 32
    carry = [[np.zeros(n, np.uint32) for _ in range(n_words)] for _ in range(qlen)]   # [row][word]
    run = np.full(n, sc.gap * qlen, dtype=np.int64)
    best = run.copy()
    score = np.full(n, sc.gap * (qlen + slen), dtype=np.int64)
    base = B * nw_block
    for blk in range(n_blocks):
        st = bitpal_init_state(nw_block, n, sc, semi) + [np.zeros(n, np.uint32) for _ in range(2 * n_words)]
        for r, ch in enumerate(query):
            for j in range(n_words):
                st[base + j] = carry[r][j].copy()
            body.simulate(st, list(peq[class_code(ch), blk * nw_block:(blk + 1) * nw_block]))
            carry[r] =[st[base + n_words + j].copy() for j in range(n_words)]
        for w in range(nw_block):
            cols = min(32, max(0, slen - 32 * (blk * nw_block + w)))
            if cols == 0:
                continue
            vals = bitpal_column_values(st, w, sc)[:, :cols]
            steps = run[:, None] + np.cumsum(vals + sc.gap, axis=1)
            best = np.maximum(best, steps.max(axis=1))
            run = steps[:, -1]
            score += vals.sum(axis=1)
    return (best if semi else score).astype(np.int16)


def bitpal_block_body(nw: int, sc: BitpalScores = BITPAL_DEFAULT):
    """Column-block form of bitpal_body: (body, initial carry-in per chain)."""
    body, init = make_blocked(bitpal_body(nw, sc), sc.planes * nw)
    return schedule(body, 200), init


def bitpal_blocked_simulate(subjects: np.ndarray, query: np.ndarray, nw_block: int,
                            sc: BitpalScores = BITPAL_DEFAULT, semi: bool = False) -> np.ndarray:
    """BitPAl over column blocks of nw_block words with carry words between blocks — the scheme of
    bitpal_blocked_kernel at toy scale.  Returns int16."""
    n, slen = subjects.shape
    qlen = len(query)
    n_blocks = -(-((slen + 31) // 32) // nw_block)
    peq = build_peq32(subjects, n_blocks * nw_block)
    body, init = bitpal_block_body(nw_block, sc)
    assert len(init) == sc.chains and not any(init)
    carry = [[np.zeros(n, np.uint32) for _ in init] for _ in range((qlen + 31) // 32)]
    run = np.full(n, sc.gap * qlen, dtype=np.int64)      # S[m][j] walking right along the last row
    best = run.copy()
    for blk in range(n_blocks):
        st = bitpal_init_state(nw_block, n, sc, semi)
        _run_block(lambda c: body.simulate(st, list(peq[c, blk * nw_block:(blk + 1) * nw_block])), st, carry, query)
        for w in range(nw_block):
            cols = min(32, max(0, slen - 32 * (blk * nw_block + w)))
            if cols == 0:
                continue
            steps = run[:, None] + np.cumsum(bitpal_column_values(st, w, sc)[:, :cols] + sc.gap, axis=1)
            best = np.maximum(best, steps.max(axis=1))
            run = steps[:, -1]
    return (best if semi else run).astype(np.int16)


# =================================================================================================
# Reference-style match masks for the simulator (32 data bits per word)
# =================================================================================================

def build_peq32(subjects: np.ndarray, nw: int, offset: int = 0) -> np.ndarray:
    """[5][nw][n_subjects] uint32, column p at bit p + offset (the banded kernels' match strings: offset = k + 1); alphabet map
    CLASS_CODE."""
    n, slen = subjects.shape
    mapped = CLASS_CODE[subjects]
    peq = np.zeros((5, nw, n), dtype=np.uint32)
    for p in range(slen):
        i = p + offset
        for c in range(5):
            peq[c, i // 32] |= ((mapped[:, p] == c).astype(np.uint32) << np.uint32(i % 32))
    return peq


def run_rows(body: Body, state: list, peq: np.ndarray, query: np.ndarray, groups: int = 1) -> None:
    planes = code_planes(peq)
    for ch in query:
        c = class_code(ch)
        body.simulate(state, list(peq[c]) * groups, cls=c, planes=planes)
