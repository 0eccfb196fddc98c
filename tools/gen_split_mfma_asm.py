#!/usr/bin/env python3
"""Generates rnnwavefunctions_amd/csrc/split_mfma_asm.h: the MFMA segment of the bf16x3 GRU step as ONE hand-scheduled
inline-asm block per K-packed layout (split_core.h, MODE 2).

Why by hand: the segment is 95 v_mfma_f32_32x32x16_bf16.  hipcc, short of registers, sinks every fragment read to just in
front of the MFMA that consumes it, so each MFMA waits out an LDS round trip (in-kernel stamps, tools/stamps.py: 51 cycles
per MFMA instead of 32).  Here the reads run ahead through a ring of two fragment sets, every wait is a counted
`s_waitcnt lgkmcnt(n)`, and nothing but MFMAs, reads and waits is issued, which leaves the SIMD's vector issue to the
partner wave's VALU segment (prnn_flip_pp_kernel).

Each weight fragment is read ONCE per block: 50 ds_read_b128 (5 tiles x 3 parts x 3 quads + 5 special) feed the 95 MFMAs.
A set is the five tiles' fragments of one (weight part, quad); all products of that set - w1: h3, h2, h1;  w2: h2, h1;
w3: h1 - are issued from the same registers, tile 0..4 per state part, so an accumulator is never written by two
consecutive MFMAs.  The sets run w3, w2, w1 (quads 0..NQ-1 inside each), then the special k-step.

Schedule: wait until the fragment has landed (first use only);  MFMA;  once the MFMA after a fragment's last one has issued,
read the fragment of the set two further on into its registers.
"""
import os
import sys

# (weight part, state parts it multiplies): one GROUP per (weight part, quad).  Groups run w3, w2, w1 and, inside a group, from
# the smallest state part to the largest, so w1 h1 of the last quad is the last regular term into every accumulator.
PARTS = [(2, (0,)), (1, (1, 0)), (0, (2, 1, 0))]


def gen_body(NT, NQ, zero=()):
    """(declarations, asm body, outputs, inputs) of one block; tiles in `zero` start from 0 (first MFMA with the inline constant
    as C, early-clobber output) instead of accumulating on their incoming value."""
    NB = 3 * NQ + 1
    # groups: (A offset of tile t, B quads the set multiplies); the special k-step is the last group, one product
    groups = []
    for p, hs in PARTS:
        for q in range(NQ):
            groups.append(([((t * 3 + p) * NQ + q) * 1024 for t in range(NT)], [h * NQ + q for h in hs]))
    groups.append(([(NT * 3 * NQ + t) * 1024 for t in range(NT)], [3 * NQ]))
    RING = 2                                   # fragment sets; set g % RING holds group g

    lines = []
    seq = {}                                   # (group, tile) -> position of its read in the wave's LDS queue
    def read(g, t):
        seq[(g, t)] = len(seq)
        lines.append("ds_read_b128 %%[f%d_%d], %%[aa] offset:%d" % (g % RING, t, groups[g][0][t]))

    for g in range(min(RING, len(groups))):
        for t in range(NT):
            read(g, t)
    started = set()
    refill = None                              # fragment whose last MFMA was the previous one
    nmfma = 0
    for g, (_, bs) in enumerate(groups):
        for i, b in enumerate(bs):
            for t in range(NT):                # always all tiles before the same accumulator again
                if i == 0:                     # LDS returns in order: at most this many younger reads still in flight
                    lines.append("s_waitcnt lgkmcnt(%d)" % (len(seq) - seq[(g, t)] - 1))
                c = "%%[c%d]" % t
                if t in zero and t not in started:
                    c = "0"
                started.add(t)
                lines.append("v_mfma_f32_32x32x16_bf16 %%[c%d], %%[f%d_%d], %%[b%d], %s" % (t, g % RING, t, b, c))
                nmfma += 1
                # the registers of a fragment are free once the MFMA AFTER its last one has issued (that last MFMA started
                # >= 32 cycles ago and has long read its operands): refill them with the group RING further on
                if refill is not None and refill[0] + RING < len(groups):
                    read(refill[0] + RING, refill[1])
                refill = (g, t) if i == len(bs) - 1 else None
    assert len(seq) == len(groups) * NT and nmfma == (6 * NQ + 1) * NT, (len(seq), nmfma)
    assert all(int(l.split("(")[1][:-1]) <= 15 for l in lines if l.startswith("s_waitcnt"))
    # the accumulators are read by VALU code right behind this block (only a barrier in between): an 8-pass MFMA's
    # result needs >= 10 wait states before a VALU read, and the assembler inserts none inside inline asm
    lines += ["s_nop 7", "s_nop 7"]
    body = "\\n\\t".join(lines).replace("%%", "%")
    ins = ", ".join(['[b%d] "v"(B[%d])' % (i, i) for i in range(NB)] + ['[aa] "v"(a_addr)'])
    decl = "u32x4 " + ", ".join("f%d_%d" % (r, t) for r in range(RING) for t in range(NT)) + ";"
    outs = ", ".join(['[c%d] "%s"(c%d)' % (t, "=&v" if t in zero else "+v", t) for t in range(NT)] +
                     ['[f%d_%d] "=&v"(f%d_%d)' % (r, t, r, t) for r in range(RING) for t in range(NT)])
    return decl, body, outs, ins


def gen(NT, NQ):
    NB = 3 * NQ + 1
    cargs = ", ".join("f32x16& c%d" % t for t in range(NT))
    ccall = ", ".join("acc[%d]" % t for t in range(NT))
    fn = '''    static __device__ __forceinline__ void %s(unsigned a_addr, const u32x4 (&B)[%d], %s) {
        %s
        asm volatile("%s"
                     : %s
                     : %s
                     : "memory");
    }
'''
    variants = ""
    for name, zero in (("run_tiles", ()), ("run_tiles_from_zero", tuple(range(NT))), ("run_tiles_zero_2_4", (2, 4))):
        decl, body, outs, ins = gen_body(NT, NQ, zero)
        variants += fn % (name, NB, cargs, decl, body, outs, ins)
    return '''template <> struct MfmaSegAsm<%d, %d> {
    static constexpr bool kAvailable = true;
    // a_addr: LDS byte address of this lane's 16 bytes in fragment 0 of the A image; B: the %d state quads
    // (3 parts x %d k-steps, then the special k-step); c0..: in = bias / one-hot rows (or the sums so far), out = pre-activations.
    // Separate accumulator references: the stacked-layer kernels run the block twice per step - X block, H block - on
    // different subsets of their seven accumulator tiles (split_pp.h: SplitPPUpper); their biases travel in two spare K entries of
    // the special k-step, so run_tiles_from_zero starts every tile from 0 (no accumulator preload, no registers held for it) and
    // run_tiles_zero_2_4 continues tiles 0, 1, 3 (r, u, mixed 0) while tiles 2, 4 (q, mixed 1 of the H block) start from 0.
%s    static __device__ __forceinline__ void run(unsigned a_addr, const u32x4 (&B)[%d], f32x16 (&acc)[%d]) {
        run_tiles(a_addr, B, %s);
    }
};
''' % (NT, NQ, NB, NQ, variants, NB, NT, ccall)


HEADER = '''// GENERATED by tools/gen_split_mfma_asm.py - do not edit (edit the generator).
// MFMA segment of the bf16x3 GRU step, hand-scheduled: every weight fragment read once, two sets ahead of its MFMAs, counted waits.
#pragma once

namespace rnnwf {

template <int NT, int NQ> struct MfmaSegAsm { static constexpr bool kAvailable = false; };

'''


def main():
    out = HEADER
    for NT, NQ in ((5, 3),):          # MODE 2 at 37..50 units: NT = 3 NF32 + NMIX = 5 tiles, NQ = 3 k-steps per part
        out += gen(NT, NQ) + "\n"
    out += "}  // namespace rnnwf\n"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              "rnnwavefunctions_amd", "csrc", "split_mfma_asm.h")
    with open(path, "w") as f:
        f.write(out)
    print("wrote", path)


if __name__ == "__main__":
    main()
