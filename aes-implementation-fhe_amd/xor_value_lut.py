"""XorValueLUT: a Zeta16 byte XOR a PUBLIC byte, decoded to its real VALUE.

The pipeline's states are nibble codes: a byte is two 16th roots of unity (hi, lo), which only a decryption can
read.  A CKKS program that wants to add, multiply or average the bytes needs them as NUMBERS.  With
zeta = e^(-2 pi i / 16) (utils.ZetaEncoder), a = zeta^k and a public nibble b,

    val(a ^ b) = sum_{p < 16} E_p[b] a^p,       E_p[b] = (1/16) sum_k (k ^ b) zeta^(-p k)      (coeffgen.xor_value_table)

and since E_0 = 7.5, E_8 is real, E_(16-p) = conj(E_p) and a^(16-p) = conj(a^p) on codewords,

    val(a ^ b) = 7.5 + E_8[b] a^8 + T + conj(T),      T = sum_{p = 1..7} E_p[b] a^p.

For a byte the output is gain * (16 val(hi ^ b_hi) + val(lo ^ b_lo)): T summed over both nibbles (14 ciphertext x
plaintext products), R = the two E_8 terms, the constant gain * 7.5 * 17 and ONE conjugation.  The powers a^1..a^8 of
hi and lo take depth 3 (7 products each, batched by xor4_lut.joint_bases), the plaintext product one more:
utils.XOR_VALUE_DEPTH = 4 levels.  With b = 0 everywhere this is the plain decode val(a); slots that hold no state
(value 1 = zeta^0, nibble 0) come out as 0.

The last XOR of counter mode has a public operand (the AES ciphertext byte), so transciphering ends here instead of
in an XOR4, a renorm and a separate decode: AESPipeline.transcipher_values.

TypedValueLUT is the same sum with per-slot weights, a signed top nibble and 16-bit words;
LinearValueLUT carries a 16 x 16 matrix per state in up to 16 weight groups.  ByteValueLUT
 decodes through an arbitrary 256-entry table of the byte instead, for one ct x ct level more;
ByteValueBank through a bank of such tables, one per slot, into several outputs of one keystream.
"""
from typing import Any, Dict

import numpy as np

from coeffgen import BYTE_LUT_Q, byte_value_table, xor_value_table
from utils import BYTE_LUT_DEPTH, XOR_VALUE_DEPTH, conj_many, mul_many
from xor4_lut import batched, joint_bases, powers

POWERS = frozenset(range(1, 9))


class XorValueLUT:
    """gain: the real number a byte value v comes out as is gain * v (default 1/256: slots in [0, 1))"""

    DEPTH = XOR_VALUE_DEPTH

    def __init__(self, ctx, gain: float = 1.0 / 256.0):
        self.ctx = ctx
        self.sc = ctx.engine.slot_count
        self.gain = float(gain)
        E = xor_value_table()[:9]
        self.tab_hi = np.ascontiguousarray(16.0 * self.gain * E)  # rows E_0..E_8 of the hi nibble, scaled by its weight
        self.tab_lo = np.ascontiguousarray(self.gain * E)
        self.const = self.gain * 7.5 * 17.0                      # E_0 of both nibbles

    def _nibbles(self, nibbles) -> np.ndarray:
        nib = np.ascontiguousarray(nibbles, dtype=np.uint8)
        if nib.shape != (self.sc,):
            raise ValueError(f"public nibbles: one uint8 per slot ({self.sc}), got shape {nib.shape}")
        if nib.size and int(nib.max()) >= 16:
            raise ValueError("public nibbles must be < 16")
        return nib

    def _bases(self, hi, lo):
        """({p: hi^p}, {p: lo^p}) for p = 1..8: the two chains' products of one depth in one multiply_many batch"""
        ctx = self.ctx
        if batched(ctx):
            return joint_bases(ctx, [(hi, POWERS, "pow"), (lo, POWERS, "pow")])
        return powers(ctx, hi, POWERS), powers(ctx, lo, POWERS)

    def _fused(self, op: str, *args):
        """the result of ONE engine call ctx.<op>(*args); None: the context has no such op, or the powers sit too
        low for it (level)"""
        ev = getattr(self.ctx, op, None)
        if ev is None or not getattr(self.ctx, "fused_luts", False):
            return None
        try:
            return ev(*args)
        except RuntimeError as e:
            if "level" in str(e):
                return None
            raise

    def _engine(self, A_hi: Dict[int, Any], A_lo: Dict[int, Any], nib_hi, nib_lo):
        """[(T, R)] from Engine.xor_value_public (one group), or None (_fused)"""
        out = self._fused("xor_value_public", A_hi, A_lo, nib_hi, nib_lo, self.tab_hi, self.tab_lo)
        return None if out is None else [out]

    def _loop(self, A_hi, A_lo, nib_hi, nib_lo):
        """[(T, R)] as the product loop over encoded per-slot coefficient vectors (XOR4LUT._public_loop's form):
        existing calls only, so it runs on any context"""
        ctx = self.ctx
        T = R = None
        for A, tab, nib in ((A_hi, self.tab_hi, nib_hi), (A_lo, self.tab_lo, nib_lo)):
            for p in range(1, 8):
                t = ctx.multiply(A[p], ctx.encode(tab[p, nib]))
                T = t if T is None else ctx.add(T, t)
            r = ctx.multiply(A[8], ctx.encode(tab[8, nib]))
            R = r if R is None else ctx.add(R, r)
        return [(T, R)]

    def apply_public(self, hi, lo, nib_hi, nib_lo):
        """ONE ciphertext whose slots hold gain * (16 (hi ^ nib_hi) + (lo ^ nib_lo)) as real numbers -- a
        TypedValueLUT: whose word slots hold gain * q + offset, q the integer the XORed bytes spell in the spec's
        dtype, and whose other slots hold 0 -- XOR_VALUE_DEPTH levels below the inputs.  hi / lo: clean Zeta16
        ciphertexts (unit magnitude, as a renorm or a fresh encryption leaves them); nib_*: the public nibble of
        every slot (uint8, slot_count entries; StateEncoder.nibble_slots).

        _engine / _loop give one (T, R) per weight group; a second group (the other byte of a 16-bit word) is
        rotated onto the first before the one conjugation."""
        ctx = self.ctx
        nib_hi, nib_lo = self._nibbles(nib_hi), self._nibbles(nib_lo)
        A_hi, A_lo = self._bases(hi, lo)
        groups = self._engine(A_hi, A_lo, nib_hi, nib_lo)
        if groups is None:
            groups = self._loop(A_hi, A_lo, nib_hi, nib_lo)
        T, R = groups[0]
        if len(groups) == 2:
            t1, r1 = self._rotate_pairs(list(groups[1]))
            T, R = ctx.add(T, t1), ctx.add(R, r1)
        return ctx.add_plain(ctx.add(ctx.add(R, T), ctx.conjugate(T)), self.const)

    def apply(self, hi, lo):
        """the plain decode gain * (16 hi + lo): apply_public with zero nibbles"""
        zero = np.zeros(self.sc, np.uint8)
        return self.apply_public(hi, lo, zero, zero)

    __call__ = apply


class TypedValueLUT(XorValueLUT):
    """The value decode to TYPED numbers: int8 / uint8 bytes or 16-bit words of either sign and
    byte order, times a per-word gain plus a per-word offset, for no level beyond XorValueLUT's four.

    The decoded value is linear in the table, so a real weight per slot scales it per slot; a signed top nibble
    is the same table with its odd rows negated (coeffgen.xor_value_table(signed=True)); and with group g's weights
    non-zero only on byte g of each word, X_0 + rotate(X_1, d) holds the word in the slot of its first byte and 0
    everywhere else -- no mask.  By linearity that is (R_0 + rot R_1) + V + conj(V) + const with V = T_0 + rot T_1:
    two rotations (one batched key switch) and one conjugation.

    spec: a state_encoder.ValueSlots (StateEncoder.value_slots((dtype, gain, offset)))."""

    MAX_GROUPS = 2

    def __init__(self, ctx, spec):
        super().__init__(ctx, 1.0)  # the unit tables 16 E and E: the weights carry the gain
        self._set_spec(spec)
        self.distance = int(spec.distance)

    def _set_spec(self, spec):
        if spec.weights.shape != (spec.groups, self.sc) or spec.flags.shape != spec.weights.shape or spec.const.shape != (self.sc,):
            raise ValueError(f"value spec: per-slot vectors of {self.sc} entries")
        if not 1 <= spec.groups <= self.MAX_GROUPS:
            raise ValueError("value spec: one or two weight groups" if self.MAX_GROUPS == 2 else f"value spec: 1..{self.MAX_GROUPS} weight groups")
        self.spec = spec
        self.weights = np.ascontiguousarray(spec.weights, np.float64)
        self.flags = np.ascontiguousarray(spec.flags, np.uint8)
        self.const = np.ascontiguousarray(spec.const, np.float64)  # per slot, unlike XorValueLUT's scalar
        E, Es = xor_value_table()[:9], xor_value_table(signed=True)[:9]
        self._tabs = (16.0 * E, 16.0 * Es, E)  # hi unsigned, hi signed, lo (the fallback's)

    def _engine(self, A_hi, A_lo, nib_hi, nib_lo):
        """[(T_g, R_g)] from Engine.xor_value_typed, or None (_fused)"""
        return self._fused("xor_value_typed", A_hi, A_lo, nib_hi, nib_lo, self.weights, self.flags if self.flags.any() else None)

    def _loop(self, A_hi, A_lo, nib_hi, nib_lo):
        """[(T_g, R_g)] as the product loop, the weights and the sign folded into the encoded coefficient vectors"""
        ctx = self.ctx
        hi_u, hi_s, lo = self._tabs
        out = []
        for w, f in zip(self.weights, self.flags):
            signed = (f & 1).astype(bool)
            T = R = None
            for A, nib, half in ((A_hi, nib_hi, 0), (A_lo, nib_lo, 1)):
                for p in range(1, 9):
                    c = lo[p, nib] if half else np.where(signed, hi_s[p, nib], hi_u[p, nib])
                    t = ctx.multiply(A[p], ctx.encode(w * c))
                    if p == 8:
                        R = t if R is None else ctx.add(R, t)
                    else:
                        T = t if T is None else ctx.add(T, t)
            out.append((T, R))
        return out

    def _rotate_pairs(self, cts):
        """[rotate(ct, -distance)]: slot j takes slot j + distance (the word's second byte onto its first), the
        independent rotations as one batched key switch where the context has it"""
        ctx = self.ctx
        multi = getattr(ctx, "rotate_multi", None)
        if multi is not None:
            return multi([(c, -self.distance) for c in cts])
        return [ctx.rotate(c, -self.distance) for c in cts]


class LinearValueLUT(TypedValueLUT):
    """The value decode with a 16 x 16 linear map over the bytes of every state fused in, for no
    level beyond XorValueLUT's four.

    §3.21's two weight groups are the diagonal method with two diagonals.  With group k weighing the slot of byte
    position p by W'[(p - k) % 16, p] * in_scale (StateEncoder.linear_slots), sum_k rotate(X_k, steps[k]) is W applied
    to the decoded bytes; by linearity that is sum_k rot(R_k) + V + conj(V) + const with V = sum_k rot(T_k).  All
    rotations of a call go through ONE rotate_multi, the conjugation is the last key switch, and an all-zero diagonal
    costs nothing: a 3-tap filter is 3 groups.

    spec: a state_encoder.LinearSlots (StateEncoder.linear_slots(W, bias, dtype, in_scale, zero_point))."""

    MAX_GROUPS = 16

    def __init__(self, ctx, spec):
        XorValueLUT.__init__(self, ctx, 1.0)  # the unit tables: the weights carry the matrix and in_scale
        self._set_spec(spec)
        if len(spec.steps) != spec.groups:
            raise ValueError("linear spec: one rotation step per weight group")
        self.steps = [int(st) for st in spec.steps]

    def _engine(self, A_hi, A_lo, nib_hi, nib_lo):
        """[(T_k, R_k)] from Engine.xor_value_groups, or None (_fused)"""
        return self._fused("xor_value_groups", A_hi, A_lo, nib_hi, nib_lo, self.weights, self.flags if self.flags.any() else None)

    def _rotate_items(self, items):
        """[rotate(ct, steps)] for all (ct, steps) of the call as one batched key switch where the context has it"""
        ctx = self.ctx
        multi = getattr(ctx, "rotate_multi", None)
        if multi is not None:
            return list(multi(items))
        return [ctx.rotate(c, st) for c, st in items]

    def apply_public(self, hi, lo, nib_hi, nib_lo):
        """ONE ciphertext whose state slots hold W (q - zero_point) * in_scale + bias, q the bytes hi ^ nib_hi,
        lo ^ nib_lo spell in the spec's dtype, and whose other slots hold 0 -- XOR_VALUE_DEPTH levels below the inputs
        (XorValueLUT.apply_public's operands)"""
        ctx = self.ctx
        nib_hi, nib_lo = self._nibbles(nib_hi), self._nibbles(nib_lo)
        A_hi, A_lo = self._bases(hi, lo)
        groups = self._engine(A_hi, A_lo, nib_hi, nib_lo)
        if groups is None:
            groups = self._loop(A_hi, A_lo, nib_hi, nib_lo)
        moved = [g for g, st in enumerate(self.steps) if st % self.sc]
        rot = iter(self._rotate_items([(c, self.steps[g]) for g in moved for c in groups[g]]))
        T = R = None
        for g, (t, r) in enumerate(groups):
            if g in moved:
                t, r = next(rot), next(rot)
            T, R = (t, r) if T is None else (ctx.add(T, t), ctx.add(R, r))
        return ctx.add_plain(ctx.add(ctx.add(R, T), ctx.conjugate(T)), self.const)


class ByteValueLUT(XorValueLUT):
    """The value decode through an arbitrary 256-entry real table f of the byte: the output slot
    holds weights * f[byte ^ public byte] -- ReLU of an int8, a G.711 sample, an sRGB pixel, an FP8 number, any 8-bit
    codebook -- exactly on the nibble code, where a polynomial of the decoded number would be deep and inexact.

    A function of a byte is a bivariate polynomial of degree < 16 in its two codewords a (hi) and c (lo), and the public
    XOR only permutes its coefficient table per slot (coeffgen.byte_value_table):
        f(x ^ b) = C_00 + T + conj(T),   T = sum_{q = -7..8} y_q U_q,   U_q = sum_{p = 0..8} K_pq[b] a^p,
    y_q = c^q (q >= 0, y_0 = 1), conj(c^-q) (q < 0).  The powers take depth 3, the plaintext products of U_q a fourth
    level and the 15 ct x ct products y_q U_q (q != 0; summed before one relinearisation) a fifth: BYTE_LUT_DEPTH = 5.
    Everything goes through T + conj(T), which also cancels imaginary noise.

    table: 256 finite reals; weights: one real per slot (StateEncoder.lut_slots: the gain on state slots, 0 elsewhere,
    so slots that hold no state come out 0)."""

    DEPTH = BYTE_LUT_DEPTH

    def __init__(self, ctx, table, weights):
        self.ctx = ctx
        self.sc = ctx.engine.slot_count
        self.K, self.c00 = byte_value_table(table)  # ValueError: not 256 finite reals
        self.table = np.asarray(table, np.float64).copy()
        w = np.asarray(weights, np.float64)
        if w.shape != (self.sc,) or not np.all(np.isfinite(w)):
            raise ValueError(f"byte table weights: one finite real per slot ({self.sc}), got shape {w.shape}")
        self.weights = np.ascontiguousarray(w)
        self.const = self.weights * self.c00

    def _engine(self, A_hi, nib_hi, nib_lo):
        """[U_q] from Engine.byte_lut_public, or None (_fused)"""
        return self._fused("byte_lut_public", A_hi, nib_hi, nib_lo, self.K, self.weights)

    def _loop(self, A_hi, nib_hi, nib_lo):
        """[U_q] as the product loop over encoded per-slot coefficient vectors: existing calls only, so it runs on any
        context.  The p = 0 column is added as a plaintext after the products"""
        ctx = self.ctx
        b = 16 * nib_hi.astype(np.int64) + nib_lo.astype(np.int64)
        out = []
        for qi in range(len(BYTE_LUT_Q)):
            U = None
            for p in range(1, 9):
                k = self.K[p, qi, b]
                if not np.any(self.K[p, qi]):
                    continue
                t = ctx.multiply(A_hi[p], ctx.encode(self.weights * k))
                U = t if U is None else ctx.add(U, t)
            if U is None:  # no table leaves a group without a hi power (p = 1..7 are dense in q), kept for safety
                U = ctx.multiply(A_hi[1], ctx.encode(np.zeros(self.sc)))
            if np.any(self.K[0, qi]):
                U = ctx.add_plain(U, self.weights * self.K[0, qi, b])
            out.append(U)
        return out

    def apply_public(self, hi, lo, nib_hi, nib_lo):
        """ONE ciphertext whose slots hold weights * table[(16 hi + lo) ^ (16 nib_hi + nib_lo)] as real numbers,
        BYTE_LUT_DEPTH levels below the inputs (XorValueLUT.apply_public's operands)"""
        ctx = self.ctx
        nib_hi, nib_lo = self._nibbles(nib_hi), self._nibbles(nib_lo)
        A_hi, A_lo = self._bases(hi, lo)
        bars = conj_many(ctx, [A_lo[k] for k in range(1, 8)])  # conj(c^1..c^7): one batched conjugation
        y = {q: A_lo[q] if q > 0 else bars[-q - 1] for q in BYTE_LUT_Q if q != 0}
        U = self._engine(A_hi, nib_hi, nib_lo)
        if U is None:
            U = self._loop(A_hi, nib_hi, nib_lo)
        T = U[BYTE_LUT_Q.index(0)]  # y_0 = 1
        for t in mul_many(ctx, [(y[q], U[qi]) for qi, q in enumerate(BYTE_LUT_Q) if q != 0]):
            T = ctx.add(T, t)
        return ctx.add_plain(ctx.add(T, ctx.conjugate(T)), self.const)


BYTE_LUT_BANK_MAX = 64  # tables per bank (the engine's kByteLutBankMax)


def bank_coefficients(tables):
    """(tables, K, c00) of a bank of byte tables: (T, 256) float64, (T, 9, 16, 256) complex and the T means
    (coeffgen.byte_value_table per table).  ValueError: not (T, 256) with 1 <= T <= 64, or a non-finite entry"""
    t = np.asarray(tables, np.float64)
    if t.ndim != 2 or t.shape[1] != 256 or not 1 <= t.shape[0] <= BYTE_LUT_BANK_MAX:
        raise ValueError(f"byte table bank: (T, 256) reals with 1 <= T <= {BYTE_LUT_BANK_MAX}, got shape {t.shape}")
    made = [byte_value_table(f) for f in t]
    return t.copy(), np.ascontiguousarray(np.stack([k for k, _ in made])), np.array([c for _, c in made], np.float64)


class ByteValueBank(XorValueLUT):
    """ByteValueLUT with a BANK of tables, a table per slot and several outputs per call: output k's
    slot j holds weights_k[j] * tables[sel_k[j]][byte ^ public byte] -- a per-channel zero point inside a non-linearity,
    a per-field codebook, eight flag bits or two int4 values of one byte.

    The ciphertext side of ByteValueLUT does not change: f(x ^ b) = C_00 + T + conj(T), T = sum_q y_q U_q,
    U_q = sum_p w K_pq[b] a^p; only the public per-slot coefficients do, slot j reading K^(sel[j]).  The power bases
    a^1..a^8 / c^1..c^8 and the seven conjugates conj(c^1..c^7) are computed ONCE per call; every output has its own
    16 sums U_q (one engine call each), its own 15 ct x ct products and its own conjugation, the products of all
    outputs in one multiply_many batch and the conjugations in one conjugate_many.  DEPTH as ByteValueLUT's.

    tables: (T, 256) finite reals, 1 <= T <= 64; outputs: K >= 1 triples (sel, weights, const) of per-slot vectors
    (StateEncoder.lut_bank_slots: sel uint8 in [0, T))."""

    DEPTH = BYTE_LUT_DEPTH

    def __init__(self, ctx, tables, outputs):
        self.ctx = ctx
        self.sc = ctx.engine.slot_count
        self.tables, self.K, self.c00 = bank_coefficients(tables)
        t = self.tables
        outputs = list(outputs)
        if not outputs:
            raise ValueError("byte table bank: at least one output (sel, weights, const)")
        self.outputs = []
        for sel, weights, const in outputs:
            s, w, c = np.asarray(sel), np.asarray(weights, np.float64), np.asarray(const, np.float64)
            if s.shape != (self.sc,) or s.dtype != np.uint8 or int(s.max()) >= len(t):
                raise ValueError(f"byte table bank: one uint8 table index < {len(t)} per slot ({self.sc}), got {s.dtype} {s.shape}")
            if w.shape != (self.sc,) or c.shape != (self.sc,) or not (np.all(np.isfinite(w)) and np.all(np.isfinite(c))):
                raise ValueError(f"byte table bank: weights and const are one finite real per slot ({self.sc})")
            self.outputs.append((np.ascontiguousarray(s), np.ascontiguousarray(w), np.ascontiguousarray(c)))

    def _engine(self, A_hi, nib_hi, nib_lo, sel, weights):
        """[U_q] of one output from Engine.byte_lut_bank_public, or None (_fused)"""
        return self._fused("byte_lut_bank_public", A_hi, nib_hi, nib_lo, self.K, sel, weights)

    def _loop(self, A_hi, nib_hi, nib_lo, sel, weights):
        """[U_q] of one output as ByteValueLUT._loop's product loop, the coefficients gathered from the slot's table"""
        ctx = self.ctx
        b = 16 * nib_hi.astype(np.int64) + nib_lo.astype(np.int64)
        t = sel.astype(np.int64)
        out = []
        for qi in range(len(BYTE_LUT_Q)):
            U = None
            for p in range(1, 9):
                if not np.any(self.K[:, p, qi]):
                    continue
                term = ctx.multiply(A_hi[p], ctx.encode(weights * self.K[t, p, qi, b]))
                U = term if U is None else ctx.add(U, term)
            if U is None:
                U = ctx.multiply(A_hi[1], ctx.encode(np.zeros(self.sc)))
            if np.any(self.K[:, 0, qi]):
                U = ctx.add_plain(U, weights * self.K[t, 0, qi, b])
            out.append(U)
        return out

    def apply_public(self, hi, lo, nib_hi, nib_lo):
        """[ciphertext k for k < K]: slot j of output k holds weights_k[j] * tables[sel_k[j]][(16 hi + lo) ^ (16 nib_hi +
        nib_lo)], BYTE_LUT_DEPTH levels below the inputs (XorValueLUT.apply_public's operands)"""
        ctx = self.ctx
        nib_hi, nib_lo = self._nibbles(nib_hi), self._nibbles(nib_lo)
        A_hi, A_lo = self._bases(hi, lo)
        bars = conj_many(ctx, [A_lo[k] for k in range(1, 8)])  # conj(c^1..c^7): one batched conjugation for all outputs
        y = {q: A_lo[q] if q > 0 else bars[-q - 1] for q in BYTE_LUT_Q if q != 0}
        Us = []
        for sel, weights, _ in self.outputs:
            U = self._engine(A_hi, nib_hi, nib_lo, sel, weights)
            Us.append(U if U is not None else self._loop(A_hi, nib_hi, nib_lo, sel, weights))
        prods = iter(mul_many(ctx, [(y[q], U[qi]) for U in Us for qi, q in enumerate(BYTE_LUT_Q) if q != 0]))  # 15 K products
        Ts = []
        for U in Us:
            T = U[BYTE_LUT_Q.index(0)]  # y_0 = 1
            for _ in range(len(BYTE_LUT_Q) - 1):
                T = ctx.add(T, next(prods))
            Ts.append(T)
        return [ctx.add_plain(ctx.add(T, bar), const) for T, bar, (_, _, const) in zip(Ts, conj_many(ctx, Ts), self.outputs)]

    def apply(self, hi, lo):
        """apply_public with zero nibbles: the tables of the bytes themselves"""
        zero = np.zeros(self.sc, np.uint8)
        return self.apply_public(hi, lo, zero, zero)

    __call__ = apply
