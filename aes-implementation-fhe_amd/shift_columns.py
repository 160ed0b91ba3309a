"""ShiftColumns: ShiftRows conjugated by the 4 x 4 transpose, the permutation of FIPS-197 mode.

With T the transpose of the column-first state (T(s)[r + 4c] = s[c + 4r]) and E' the pipeline's round sequence
with SC = T . ShiftRows . T in place of ShiftRows, fips_encrypt(p, rks) = T(E'(T p, [T rk_r])): the row-mixing
MixColumns of this project is the transpose-conjugate of FIPS-197's, SubBytes and AddRoundKey
are byte-wise, so only the permutation changes (AESPipeline(fips=True)).  SC(s)[r + 4c] = s[((r + c) % 4) + 4c]:
column c (bytes 4c .. 4c + 3) rotated by c inside itself; the inverse rotates it back.

ShiftRows moves whole rows by multiples of 4 units, which a 16-unit-periodic state wraps; SC moves bytes inside
groups of 4, which no 1-D slot layout makes cyclic, so every cell class reads its own offset: 7 offsets
{0, +-1, +-2, +-3} units per half.  The sum of masked rotations is ONE ctx.rot_pt_sum call per half (the engine's
double-hoisted aesfhe_rot_pt_sum); MixColFinal.sr_entry takes the 11-step form built by
entry_terms.  No reference counterpart (REF/shift_rows.py:7-56 is the row form).
"""
from typing import Any, List

import numpy as np

SC_PERM = [0, 1, 2, 3, 5, 6, 7, 4, 10, 11, 8, 9, 15, 12, 13, 14]      # output byte i takes input byte SC_PERM[i]
INV_SC_PERM = [0, 1, 2, 3, 7, 4, 5, 6, 10, 11, 8, 9, 13, 14, 15, 12]


def transpose_bytes(state: np.ndarray) -> np.ndarray:
    """T on a (16,) or (..., 16) column-first state: T(s)[r + 4c] = s[c + 4r] (an involution)"""
    s = np.asarray(state, np.uint8)
    return np.ascontiguousarray(np.swapaxes(s.reshape(*s.shape[:-1], 4, 4), -1, -2)).reshape(s.shape)


def _perm(direction: int) -> List[int]:
    """output byte i = r + 4c takes input byte ((r - direction * c) % 4) + 4c"""
    return [((i % 4 - direction * (i // 4)) % 4) + 4 * (i // 4) for i in range(16)]


def shift_columns_bytes(state: np.ndarray, direction: int = -1) -> np.ndarray:
    """the byte permutation ShiftColumns (direction -1) / InvShiftColumns (+1) applies to a (16,) or (B, 16)
    column-first state: column c rotated by -direction * c positions inside itself"""
    s = np.asarray(state, np.uint8)
    return s[..., _perm(direction)]


def cell_offset(i: int, direction: int = -1) -> int:
    """units between the input byte output byte i takes and i itself, in -3 .. 3"""
    return _perm(direction)[i] - i


def apply_terms(layout, direction: int = -1):
    """(steps, masks): the 7 masked rotations of one half, out = sum_k masks[k] * np.roll(x, steps[k])"""
    steps, masks = [], []
    for d in range(-3, 4):
        m = np.zeros(layout.sc)
        for i in range(16):
            if cell_offset(i, direction) == d:
                m += layout.cell_mask(i % 4, i // 4).real
        steps.append(-d * layout.unit)  # np.roll(x, s)[j] = x[j - s]: the byte d units above
        masks.append(m)
    return steps, masks


def entry_terms(layout, direction: int = -1):
    """MixColFinal.sr_entry's form: (steps, masks) with 11 steps and masks[h][o][k] (h: the hi / lo half, o: the
    output, k: the step; None = absent) such that, for a period-periodic pair (x_0, x_1) and s1 = -4 unit,
        pack(SC(x))          = sum_h sum_k masks[h][0][k] * np.roll(x_h, steps[k])
        pack(rot(SC(x), s1)) = sum_h sum_k masks[h][1][k] * np.roll(x_h, steps[k])
    pack's half masks are folded into the cell masks.  Output 0 reads offsets -3 .. 3 units; output 1's byte i is
    SC(x)'s byte i + 4 (mod 16, the state being 16-unit-periodic), i.e. x's byte i + 4 + offset(i + 4): offsets
    1 .. 7 units.  Together 11 offsets, 10 of them rotations, 7 masked terms per half and output."""
    if not layout.packable:
        raise ValueError("entry_terms: the packed form needs the periodic layout with 2 * period <= slot count")
    offs = list(range(-3, 8))
    steps = [-d * layout.unit for d in offs]
    halves = [layout.half_mask(h).real for h in (0, 1)]
    cell = [layout.cell_mask(i % 4, i // 4).real for i in range(16)]
    masks = []
    for h in (0, 1):
        per_out = []
        for o in (0, 1):
            row = []
            for d in offs:
                m = np.zeros(layout.sc)
                for i in range(16):
                    src = (i + 4 * o) % 16
                    if 4 * o + cell_offset(src, direction) == d:
                        m += cell[i]
                row.append(m * halves[h] if m.any() else None)
            per_out.append(row)
        masks.append(per_out)
    return steps, masks


class ShiftColumns:
    """the interface of shift_rows.ShiftRows (ctx, states, layout; apply, slot_perm, direction, layout)"""
    direction = -1
    column_form = True  # MixColFinal.sr_entry: the 11-step rot_pt_sum form instead of ShiftRows' R^4 = id form

    def __init__(self, ctx, states: int = 1, layout=None):
        from state_encoder import SlotLayout
        self.ctx = ctx
        self.sc = ctx.engine.slot_count
        self.layout = layout or SlotLayout(self.sc, states)
        self.stride = self.layout.unit
        self.states = states
        if getattr(ctx, "rot_pt_sum", None) is None:
            raise TypeError("ShiftColumns needs a context with rot_pt_sum (engine_context.EngineContext)")
        self._rot_steps, masks = apply_terms(self.layout, self.direction)
        self._pt_masks = [ctx.encode(m) for m in masks]

    def slot_perm(self):
        """output slot i <- input slot perm[i] for the one-state periodic layout (byte i in slot i), else None:
        what a renorm folds (StateEncoder.renorm_perm, FOLDS.sr), as ShiftRows.slot_perm"""
        if not (self.layout.periodic and self.stride == 1 and self.layout.period == 16):
            return None
        return _perm(self.direction)

    def _apply_one(self, ct: Any) -> Any:
        return self.ctx.rot_pt_sum(ct, self._rot_steps, [self._pt_masks])[0]

    def apply(self, ct_hi: Any, ct_lo: Any):
        """both halves: 7 masked rotations each as one double-hoisted sum, one level"""
        return self._apply_one(ct_hi), self._apply_one(ct_lo)


class InvShiftColumns(ShiftColumns):
    direction = +1
