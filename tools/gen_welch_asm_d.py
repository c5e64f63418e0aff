#!/usr/bin/env python3
"""Generator (and CPU emulator) of `mdsp_welch_w64d_asm`: the carried-half-frame Welch kernel of tools/gen_welch_asm_c.py with FEWER VECTOR INSTRUCTIONS.

The kernel runs at the package power cap: its time follows the energy of its vector instructions (leaving out the 128 power FMAs of a unit, 8 % of them,
took 1.314 ms to 1.263 ms).  Same loads, banks, exchange and arguments as mdsp_welch_w64c_asm; what changes is the arithmetic:
  * FMA-folded twiddled butterflies.  A twiddled value w b that meets its partner a is never formed: y0 = a + w b is two v_pk_fma_f32 (b.y and b.x
    broadcast by op_sel against w with its halves swapped / negated as needed) and y1 = a - w b = 2 a - y0 one more (the 2 in an SGPR pair): 3
    instructions instead of cmul + add + sub = 4.  Powers of -i on a twiddle are modifiers, so the SGPR pairs hold W64^r for r = 1..15 only.
  * pass A's second layer and pass B's first layer fold the twiddles of the upper half of each radix-8 (j + 4) into its first radix-2 stage;
  * pass B's second layer takes W^(lane t1) and the tail's W64^(t1 k1) as ONE twiddle, c^t1 with c = W^(lane + 64 k1), and factors its powers
    through the radix-8 (DIT: E = bfly4 of (x0, d x2, e x4, d e x6), d = c^2, e = c^4, likewise O, then Y[k] = E[k] +- W8^k c O[k]): 12 folds and
    the four per-lane values c, d, e, g = W8 c, read from LDS for k1 < 4 and, for k1 + 4, one product each of the same four (kept in registers:
    k1 and k1 + 4 are transformed back to back) with W64^4, W64^8, W64^4 (e: a rotation by -i).  The 56 products behind pass B's first layer
    disappear;
  * that layer's last radix-2 stage never forms its outputs: p = w O, then (E.x + p.x, E.x - p.x) and (E.y + p.y, E.y - p.y) as pairs, squared into
    an accumulator PAIR holding bins k and k + 4 (acc_reg): 6 instructions where the fold and four v_fma_f32 took 7;
  * pass A's second layer takes the factored form too where it is cheaper (W64 constants: a rotation costs nothing there).
Per unit: 1306 vector ALU instructions against 1506 (-13 %), 119 LDS reads against 110.  The fold changes the rounding by one fused rounding per term
and y1 carries the rounding of y0: `--check` reports the relative error against numpy (1.3e-7, variant 43: 1.2e-7).

    python tools/gen_welch_asm_d.py [--check] [--ablate loads,lds,perm,acc]      writes dsp.jl_amd/csrc/welch_w64d_asm.s
Kernel contract: gen_welch_asm_c.py's (same W64AsmArgs, partial rows, grid, flush rule), with 16 more per-lane rows in the prepared block behind the
28 x 64 floats of tw (welch_w64.h w64asm_prepare_kernel): W^m, W^(2m), W^(4m), W^(m + 512), m = lane + 64 k1, k1 = 0..3.  LDS: 23 twiddle rows,
11.5 KiB, in front of the window pairs 16 KiB + 8 x 16.5 KiB exchange buffers (159.5 of 160 KiB).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_welch_asm as W
import gen_welch_asm_c as C
from gen_welch_asm import N, XBUF_BYTES, XROW

TW_ROWS = 23
TW_BYTES = TW_ROWS * 512
WIN_OFF = TW_BYTES
XB_OFF = TW_BYTES + W.WIN_BYTES
LDS_BYTES = XB_OFF + 8 * XBUF_BYTES
assert LDS_BYTES <= 160 * 1024
ROW_WA = 0         # rows 0..6: W^(8 lane j), j = 1..7 (pass B, first layer)
ROW_C = 7          # rows 7 + 4 k1 + (0, 1, 2, 3), k1 = 0..3: c, c^2, c^4, W8 c with c = W^(lane + 64 k1) (pass B, second layer)
PREP_OFF = 28 * 64 * 4     # those 16 rows in the prepared block: behind the 28 floats per lane of mdsp_welch_w64c_asm, row-major


# A twiddle operand: (src, q) = (-i)^q src, src a Val (per-lane pair) or ('s', pair) (W64 constant); q rotates for free through op_sel / neg.
# Its components: w.x = sx src[px], w.y = sy src[py].
ROT = {0: (0, 1, 1, 1), 1: (1, 1, 0, -1), 2: (0, -1, 1, -1), 3: (1, -1, 0, 1)}     # q -> (px, sx, py, sy)


def rot(tw, q):
    return (tw[0], (tw[1] + q) & 3)


class GenD(C.GenC):
    NAME = "mdsp_welch_w64d_asm"
    SCRIPT = "tools/gen_welch_asm_d.py"
    LDS_BYTES = LDS_BYTES
    WIN_OFF = WIN_OFF
    XB_OFF = XB_OFF
    S_TWO = 72     # (2, 2): y1 = 2 a - y0
    W_EXPS = list(range(1, 16))    # W64^r, r = 1..15 at s[42 + 2 (r - 1)]; W64^(16 q + r) = (-i)^q W64^r

    @staticmethod
    def tw_rows(lane):
        roots = np.exp(-2j * np.pi * np.arange(N) / N)
        rows = [roots[(8 * lane * j) % N] for j in range(1, 8)]
        for k1 in range(4):
            m = lane + 64 * k1
            rows += [roots[m % N], roots[(2 * m) % N], roots[(4 * m) % N], roots[(m + 512) % N]]
        return rows

    @classmethod
    def emit_tw_prologue(cls, A):
        A("\tv_mul_u32_u24_e32 v4, 112, v1                ; per-lane twiddles: W^(8 lane j) = the first 14 of 28 floats at tw + lane * 112, ...")
        for k in range(4):
            A(f"\tglobal_load_dwordx4 v[{cls.POOL0 + 4 * k}:{cls.POOL0 + 4 * k + 3}], v4, s[10:11] offset:{16 * k}")
        A("\tv_lshlrev_b32_e32 v7, 3, v1                  ; lane * 8")
        A(f"\tv_add_u32_e32 v5, {PREP_OFF}, v7             ; ... then 16 rows of 64 pairs at tw + {PREP_OFF}")
        A("\tv_add_u32_e32 v6, 0x1000, v5")
        for r in range(16):
            A(f"\tglobal_load_dwordx2 v[{cls.POOL0 + 16 + 2 * r}:{cls.POOL0 + 17 + 2 * r}], v{5 + r // 8}, s[10:11] offset:{512 * (r % 8)}")
        A("\ts_waitcnt vmcnt(20)")
        A(f"\tds_write_b128 v3, v[8:11] offset:{WIN_OFF}")
        A(f"\tds_write_b128 v3, v[12:15] offset:{WIN_OFF + 16}")
        A("\ts_waitcnt vmcnt(0)")
        for k in range(7):
            A(f"\tds_write_b64 v7, v[{cls.POOL0 + 2 * k}:{cls.POOL0 + 2 * k + 1}] offset:{512 * k}      ; every wave writes the same {TW_ROWS} rows")
        for r in range(16):
            A(f"\tds_write_b64 v7, v[{cls.POOL0 + 16 + 2 * r}:{cls.POOL0 + 17 + 2 * r}] offset:{512 * (7 + r)}")

    def sconsts(self):
        sc = W.sconsts(self)
        sc[self.S_TWO] = (np.float32(2.0), np.float32(2.0))
        return sc

    def emit_sconsts(self, A, fbits):
        super().emit_sconsts(A, fbits)
        A(f"\ts_mov_b32 s{self.S_TWO}, {fbits(2.0)}")
        A(f"\ts_mov_b32 s{self.S_TWO + 1}, {fbits(2.0)}")

    def trial(self, f):
        """instructions f() would emit"""
        n0 = len(self.ins)
        f()
        n = len(self.ins) - n0
        del self.ins[n0:]
        return n

    # ---- twiddles
    def w64c(self, m):
        """W64^m as a twiddle operand, None for 1"""
        m &= 63
        q, r = divmod(m, 16)
        return (None if r == 0 else ("s", self.wexp[r]), q) if m else None

    def cmul_tw(self, a, tw):
        """a w, w = (src, q); two instructions (one for a bare power of -i)"""
        src, q = tw
        if src is None:
            assert q, "a product by 1 is not emitted"
            sel = {1: ([1, 0], [0, 1]), 2: ([0, 1], [1, 1]), 3: ([1, 1], [0, 0])}[q]     # a (1, -1) with halves picked: -i a, -a, i a
            return self.pk("v_pk_mul_f32", [a, ("s", self.S_PM)], {"op_sel": sel[0], "op_sel_hi": sel[1]})
        px, sx, py, sy = ROT[q]
        t = self.pk("v_pk_mul_f32", [a, src], {"op_sel": [1, py], "op_sel_hi": [1, px], "neg_lo": [int(sy < 0), 0], "neg_hi": [int(sx < 0), 0]})
        return self.pk("v_pk_fma_f32", [a, src, t], {"op_sel": [0, px, 0], "op_sel_hi": [0, py, 1], "neg_lo": [int(sx < 0), 0, 1], "neg_hi": [int(sy < 0), 0, 0]},
                       dst=t)

    def fold(self, a, b, tw):
        """(a + w b, a - w b): three instructions for a general w, two for a power of -i, nothing but the add / sub pair for w = 1"""
        if tw is None:
            return self.add(a, b), self.sub(a, b)
        src, q = tw
        if src is None:           # a - i b, a + i b / a - b, a + b / a + i b, a - i b
            f0, f1 = {1: (self.sub_ib, self.add_ib), 2: (self.sub, self.add), 3: (self.add_ib, self.sub_ib)}[q]
            return f0(a, b), f1(a, b)
        px, sx, py, sy = ROT[q]
        # t = (a.x - w.y b.y, a.y + w.x b.y);  y0 = (t.x + w.x b.x, t.y + w.y b.x);  y1 = 2 a - y0
        t = self.pk("v_pk_fma_f32", [b, src, a], {"op_sel": [1, py, 0], "op_sel_hi": [1, px, 1], "neg_lo": [int(sy > 0), 0, 0], "neg_hi": [int(sx < 0), 0, 0]})
        y0 = self.pk("v_pk_fma_f32", [b, src, t], {"op_sel": [0, px, 0], "op_sel_hi": [0, py, 1], "neg_lo": [int(sx < 0), 0, 0], "neg_hi": [int(sy < 0), 0, 0]},
                     dst=t)
        y1 = self.pk("v_pk_fma_f32", [a, ("s", self.S_TWO), y0], {"neg_lo": [0, 0, 1], "neg_hi": [0, 0, 1]})
        return y0, y1

    def bfly8_tw(self, x, tw, pre=None):
        """out[k] = sum_j W8^(jk) w_j x_j (tw[j]: twiddle operand or None); the lower half's products first (or given in pre), the upper half's folded"""
        S, D = [], []
        for j in range(4):
            p = pre[j] if pre is not None else (x[j] if tw[j] is None else self.cmul_tw(x[j], tw[j]))
            s_, d_ = self.fold(p, x[j + 4], tw[j + 4])
            S.append(s_)
            D.append(d_)
        return self.bfly8_sd(S, D)

    def acc_reg(self, s):
        """v[s] and v[s + 4] (s = k2 + 8 k1, k2 < 4) share an accumulator pair: the power of the last radix-2 stage is accumulated packed"""
        k1, k2 = divmod(s, 8)
        return self.ACC0 + 8 * k1 + 2 * (k2 & 3) + (k2 >> 2)

    def fold_power(self, a, b, tw, acc):
        """acc += (|a + w b|^2, |a - w b|^2), acc a physical pair: p = w b, then (re, re) and (im, im) of the two as pairs, squared into acc --
        six instructions where the fold and four v_fma_f32 took seven"""
        p = self.cmul_tw(b, tw)
        re = self.pk("v_pk_fma_f32", [p, ("s", self.S_PM), a], {"op_sel": [0, 0, 0], "op_sel_hi": [0, 1, 0]})      # (a.x + p.x, a.x - p.x)
        im = self.pk("v_pk_fma_f32", [p, ("s", self.S_PM), a], {"op_sel": [1, 0, 1], "op_sel_hi": [1, 1, 1]})      # (a.y + p.y, a.y - p.y)
        for t in (re, im):
            self.emit("v_pk_fma_f32", acc, [("v", t.p), ("v", t.p), acc], {"op_sel": [0, 0, 0], "op_sel_hi": [1, 1, 1], "neg_lo": [0, 0, 0], "neg_hi": [0, 0, 0]})

    def bfly8_pow(self, x, c, d, e, g, acc=None):
        """out[k] = sum_j W8^(jk) c^j x_j with d = c^2, e = c^4, g = W8 c (twiddle operands): radix-2 DIT with the powers of c factored out, 12 folds;
        with acc(k) (the accumulator pair of outputs k, k + 4) the last stage accumulates |out[k]|^2 instead of returning out"""
        def half(y):              # (y0, d y1, e y2, d e y3) -> bfly4
            ap, am = self.fold(y[0], y[2], e)
            bp, bm = self.fold(y[1], y[3], e)
            e0, e2 = self.fold(ap, bp, d)
            e1, e3 = self.fold(am, bm, rot(d, 1))
            return [e0, e1, e2, e3]
        E = half(x[0::2])
        O = half(x[1::2])
        out = [None] * 8
        for k, w in ((0, c), (2, rot(c, 1)), (1, g), (3, rot(g, 1))):
            if acc is None:
                out[k], out[k + 4] = self.fold(E[k], O[k], w)
            else:
                self.fold_power(E[k], O[k], w, acc(k))
        return out

    def emit_unit(self):
        hh = self.hh_layout()
        c, n = self.parity, 1 - self.parity
        v = [None] * 64
        self.comment("pass A, first layer (window folded in) + first radix-8 layer; H0 from the carried bank, H2 from the new one")
        for n1 in range(8):
            wp = [self.ds_read(self.V_WIN, WIN_OFF + 512 * (n1 + 8 * j)) for j in range(4)]
            S, D = [], []
            for j in range(4):
                e = n1 + 8 * j
                h = j & 1
                T = self.alloc()
                self.emit("v_mul_f32", ("h", T.p, 0), [self.cval(c, e), ("h", wp[j].p, 0)])
                self.emit("v_mul_f32", ("h", T.p, 1), [self.cval(n, e), ("h", wp[j].p, 1)])
                s_ = self.pk("v_pk_fma_f32", [hh[n1][j >> 1], wp[j], T], {"op_sel": [h, 1, 0], "op_sel_hi": [h, 0, 1]})
                d_ = self.pk("v_pk_fma_f32", [hh[n1][j >> 1], wp[j], T],
                             {"op_sel": [h, 1, 0], "op_sel_hi": [h, 0, 1], "neg_lo": [1, 0, 0], "neg_hi": [0, 0, 1]}, dst=T)
                S.append(s_)
                D.append(d_)
            o = self.bfly8_sd(S, D)
            for k1 in range(8):
                v[n1 + 8 * k1] = o[k1]
        self.comment("pass A, second radix-8 layer (W64 twiddles of the upper half folded); half exchange by lane swaps; round 0 of the 64 x 64 transposition")
        m = [None] * 64
        for k1 in range(8):
            u = [v[j + 8 * k1] for j in range(8)]
            naive = lambda: self.bfly8_tw(u, [self.w64c(j * k1) for j in range(8)])              # noqa: E731
            fact = lambda: self.bfly8_pow(u, *(self.w64c(m) for m in (k1, 2 * k1, 4 * k1, k1 + 8)))   # noqa: E731
            out = (fact if k1 and self.trial(fact) < self.trial(naive) else naive)()
            for k2 in range(4):
                lo_, hi_ = out[k2], out[k2 + 4]
                for half in ("lo", "hi"):
                    self.emit("v_permlane32_swap", None, [getattr(lo_, half), getattr(hi_, half)])
                m[k1 + 8 * k2] = lo_
                m[k1 + 8 * (k2 + 4)] = hi_
            for k2 in range(4):
                self.ds_write(self.V_XW, 8 * (k1 + 8 * k2), m[k1 + 8 * k2])
        nv = [None] * 64
        order = sorted(range(32), key=lambda T: (T & 7, T >> 3))
        for T in order:
            nv[T] = self.ds_read(self.V_XR, 8 * XROW * T)
        for r in range(32):
            self.ds_write(self.V_XW, 8 * r, m[32 + r])
        for T in order:
            nv[32 + T] = self.ds_read(self.V_XR, 8 * XROW * T)
        v = nv
        self.comment("pass B, first radix-8 layer: W^(8 lane t2) on round 0's operands (t2 < 4) first, those of round 1 folded into the first radix-2 stage")
        pre = {}
        for t2 in (1, 2, 3):
            wa = self.ds_read(self.V_WIN, 512 * (ROW_WA + t2 - 1))
            for t1 in range(8):
                pre[(t1, t2)] = self.cmul_tw(v[t1 + 8 * t2], (wa, 0))
        wa = {t2: (self.ds_read(self.V_WIN, 512 * (ROW_WA + t2 - 1)), 0) for t2 in (4, 5, 6, 7)}
        x = [[None] * 8 for _ in range(8)]      # x[k1][t1]: the second layer's operands
        for t1 in range(8):
            out = self.bfly8_tw([v[t1 + 8 * t2] for t2 in range(8)], [None, None, None, None] + [wa[t2] for t2 in (4, 5, 6, 7)],
                                pre=[v[t1]] + [pre[(t1, t2)] for t2 in (1, 2, 3)])
            for k1 in range(8):
                x[k1][t1] = out[k1]
        self.comment("pass B, second radix-8 layer: one twiddle c^t1, c = W^(lane + 64 k1), powers factored; c, c^2, c^4, W8 c from LDS for k1 < 4, times")
        self.comment("W64^4, W64^8, -i, W64^4 for k1 + 4; the last radix-2 stage accumulates the power of its two outputs as one pair")
        for k1 in range(4):
            base = [(self.ds_read(self.V_WIN, 512 * (ROW_C + 4 * k1 + q)), 0) for q in range(4)]
            derived = []
            for w, mult in zip(base, (4, 8, 16, 4)):
                m = self.w64c(mult)
                derived.append(rot(w, m[1]) if m[0] is None else (self.cmul_tw(w[0], m), 0))
            for kk, tw in ((k1, base), (k1 + 4, derived)):
                self.bfly8_pow(x[kk], *tw, acc=lambda k, kk=kk: ("v", self.acc_reg(k + 8 * kk)))

def check():
    return C.check(GenD)


def kernel_text():
    return C.kernel_text(GenD)


if __name__ == "__main__":
    if "--check" in sys.argv:
        sys.exit(0 if check() else 1)
    if "--ablate" in sys.argv:
        W.ABLATE.update(sys.argv[sys.argv.index("--ablate") + 1].split(","))
    text, nbody = kernel_text()
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsp.jl_amd", "csrc", "welch_w64d_asm.s")
    open(out, "w").write(text)
    print(f"wrote {out}: {text.count(chr(10))} lines, {nbody} instructions per unit")
