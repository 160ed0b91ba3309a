"""StateEncoder: 16-byte AES state <-> (ct_hi, ct_lo) (REF/state_encoder.py:9-38).

Byte i (column-first order, REF/README.md:103-104) goes to slot i*stride with
stride = slot_count/16; every other slot holds 1+0j.

``states`` > 1 selects the slot-packed layout (the paper's layout in
REF/main.py:121-140): state b of a batch of B <= stride states holds byte i in slot
i*stride + b.  Every rotation the AES modules issue is a multiple of stride, so the B
columns never mix; slots with (j mod stride) >= B hold 1+0j as in the reference.
``encode`` then takes a (B, 16) uint8 array and ``decode`` returns one.

``periodic=True`` (the pipeline's default) packs the same bytes with rotation
unit B instead of stride: byte i of state b in slot i*B + b, and that 16B-slot block repeated
over all slots.  Every AES step is slot-wise or a rotation by a multiple of the unit, so the
message stays 16B-periodic -- a polynomial in the subring Z[X^(N/32B)] -- and the final
bootstraps of MixColumns / InvMixColumns run as sparse-slot bootstraps (aesfhe_bootstrap_pair_sparse,
a trace plus period-sized transforms).  Decoded states are the same in both layouts.

The two layouts are NOT interchangeable on ciphertexts: the encoder tags what it produces with
its layout (``tag_layout``) and ``decode`` / ``renorm`` / ``AESPipeline.decrypt`` refuse a
ciphertext tagged with the other one (``check_layout``).  ``StateEncoder(ctx, B)``
keeps the reference layout; ``AESPipeline`` picks the periodic one where the context has the
sparse bootstrap (its ``layout`` attribute says which).
"""
import os
from typing import Any, Tuple

import numpy as np

from utils import FOLDS, ConjSum, ZetaEncoder, conj_sum, takes_kw, tally_renorm

# AESFHE_RENORM_FRESH=1: ignore renorm target levels (A/B measurements of DESIGN.md §3.11)
_RENORM_FRESH = os.environ.get("AESFHE_RENORM_FRESH") == "1"


class SlotLayout:
    """Where the bytes of B states sit: the reference layout (byte i of state b in slot
    i*stride + b, stride = slot_count/16, every other slot 1) or the periodic one (unit = B, the
    16B-slot block repeated).  `unit` is the rotation unit of ShiftRows / MixColumns."""

    def __init__(self, sc: int, states: int = 1, periodic: bool = False):
        if not 1 <= states <= sc // 16:
            raise ValueError(f"states per ciphertext must be in [1, {sc // 16}], got {states}")
        if periodic and states & (states - 1):
            raise ValueError("the periodic layout needs a power-of-two number of states")
        self.sc, self.states, self.periodic = sc, states, periodic
        self.unit = states if periodic else sc // 16
        self.period = 16 * self.unit

    @property
    def boot_period(self):
        """the slot period a sparse bootstrap may use (None: the full-slot bootstrap)"""
        return self.period if self.period < self.sc else None

    @property
    def renorm_states(self) -> int:
        """the engine renorm's `states` (periodic: every slot holds state data)"""
        return self.sc // 16 if self.periodic else self.states

    def tile(self, block: np.ndarray) -> np.ndarray:
        return np.tile(block, self.sc // self.period)

    def row_mask(self, r: int) -> np.ndarray:
        """ones on row r (bytes r + 4c) of every state"""
        m = np.zeros(self.period, dtype=np.complex128)
        for c in range(4):
            m[(r + 4 * c) * self.unit:(r + 4 * c) * self.unit + self.states] = 1.0
        return self.tile(m)

    def cell_mask(self, r: int, c: int) -> np.ndarray:
        """ones on byte r + 4c of every state (the row masks split by column: shift_columns.py)"""
        m = np.zeros(self.period, dtype=np.complex128)
        m[(r + 4 * c) * self.unit:(r + 4 * c) * self.unit + self.states] = 1.0
        return self.tile(m)

    @property
    def packable(self) -> bool:
        """hi and lo fit side by side in one ciphertext: the packed form holds the
        hi nibbles in slots (j mod 2P) < P and the lo nibbles in the others (P = period)"""
        return self.periodic and 2 * self.period <= self.sc

    def half_mask(self, which: int) -> np.ndarray:
        """ones on the hi (0) / lo (1) half of every 2P-slot block of the packed form"""
        m = np.zeros(2 * self.period, dtype=np.complex128)
        m[which * self.period:(which + 1) * self.period] = 1.0
        return np.tile(m, self.sc // (2 * self.period))

    # "transposed": the ciphertexts hold T(state) (shift_columns.transpose_bytes; AESPipeline(fips=True)) -- part
    # of the tag check_layout compares, so a transposed pair never meets a plain pipeline or encoder
    byte_order = "plain"

    def same(self, other) -> bool:
        return other is not None and (self.sc, self.states, self.periodic, self.byte_order) == (
            other.sc, other.states, other.periodic, getattr(other, "byte_order", "plain"))


def tag_layout(layout: SlotLayout, *cts):
    """mark ciphertexts as holding states in `layout` (checked by check_layout); returns them"""
    for c in cts:
        try:
            c.layout = layout
        except AttributeError:  # a context whose ciphertexts carry no tag (the CPU oracle's)
            pass
    return cts


def dump_ct(ctx, ct):
    """(array, level, layout) of a ciphertext for the wire between a client and a server context:
    its residues [npoly][limbs][N] uint32, its level, and its slot-layout tag as a plain dict (None: untagged), so a
    pipeline pair keeps ct.layout across the transport"""
    lay = getattr(ct, "layout", None)
    tag = None if lay is None else dict(sc=int(lay.sc), states=int(lay.states), periodic=bool(lay.periodic),
                                        byte_order=str(getattr(lay, "byte_order", "plain")))
    return ctx.engine.export(ct), int(ct.level), tag


def load_ct(ctx, array, level: int, layout=None, check: bool = True):
    """the ciphertext dump_ct wrote, imported into `ctx` and tagged with its layout again.  check=True (the default
    for anything that crossed a wire) runs the engine's residue check first: a word not below its limb's modulus is
    refused with ValueError before any arithmetic kernel sees the data"""
    if layout is not None and int(layout["sc"]) != ctx.engine.slot_count:
        raise ValueError(f"load_ct: a layout of {layout['sc']} slots into a context of {ctx.engine.slot_count}")
    ct = ctx.engine.import_ct(np.asarray(array), int(level))
    if check:
        bad = ctx.engine.check(ct)
        if bad is not None:
            raise ValueError(f"load_ct: residue not below its modulus in row {bad}")
    if layout is not None:
        lay = SlotLayout(int(layout["sc"]), int(layout["states"]), bool(layout["periodic"]))
        lay.byte_order = str(layout.get("byte_order", "plain"))
        tag_layout(lay, ct)
    return ct


def _layout_tag(ct):
    lay = getattr(ct, "layout", None)
    return None if lay is None else dict(sc=int(lay.sc), states=int(lay.states), periodic=bool(lay.periodic),
                                         byte_order=str(getattr(lay, "byte_order", "plain")))


def _layout_of_tag(layout) -> SlotLayout:
    """the SlotLayout a _layout_tag dict describes"""
    lay = SlotLayout(int(layout["sc"]), int(layout["states"]), bool(layout["periodic"]))
    lay.byte_order = str(layout.get("byte_order", "plain"))
    return lay


def _layout_of(ctx, layout, who: str):
    if layout is None:
        return None
    if int(layout["sc"]) != ctx.engine.slot_count:
        raise ValueError(f"{who}: a layout of {layout['sc']} slots into a context of {ctx.engine.slot_count}")
    lay = SlotLayout(int(layout["sc"]), int(layout["states"]), bool(layout["periodic"]))
    lay.byte_order = str(layout.get("byte_order", "plain"))
    return lay


def dump_ct_seeded(ctx, ct):
    """(b_rows, level, layout, seed_id) of a seeded fresh ciphertext (ctx.encrypt_seeded): half of
    dump_ct's bytes, the a rows being a public function of seed_id and the context's mask key.  Any other ciphertext
    (an operation's result, a public-key encryption) is refused by the engine: "not a seeded ciphertext\""""
    b, sid = ctx.engine.export_half(ct)
    return b, int(ct.level), _layout_tag(ct), sid


def load_ct_seeded(ctx, b_rows, level: int, seed_id: int, layout=None):
    """the ciphertext dump_ct_seeded wrote, completed on `ctx`'s device (any context holding the sender's mask key, an
    evaluation-only one included): the b rows are checked as load_ct(check=True) checks them, the a rows regenerated"""
    return load_cts_seeded(ctx, [(b_rows, level, layout, seed_id)])[0]


def load_cts_seeded(ctx, records):
    """load_ct_seeded of several dump_ct_seeded records; runs of one level and consecutive seed ids (the members of
    one encrypt_seeded_many call, in order) go through one batched import each"""
    records = list(records)
    lays = [_layout_of(ctx, r[2], "load_ct_seeded") for r in records]
    for r in records:
        if np.asarray(r[0]).ndim != 2:
            raise ValueError("load_ct_seeded: b rows are [limbs][N]")
    out, i = [], 0
    while i < len(records):
        j = i + 1
        while (j < len(records) and int(records[j][1]) == int(records[i][1])
               and int(records[j][3]) == int(records[i][3]) + ((j - i) << 16)
               and np.asarray(records[j][0]).shape == np.asarray(records[i][0]).shape):
            j += 1
        out += ctx.engine.import_half_many([r[0] for r in records[i:j]], int(records[i][1]), int(records[i][3]))
        i = j
    for ct, lay in zip(out, lays):
        if lay is not None:
            tag_layout(lay, ct)
    return out


def check_layout(layout: SlotLayout, *cts) -> None:
    """raise if a ciphertext was tagged with another slot layout (a pair made by an encoder with
    the reference layout decrypts to wrong bytes under the periodic one, and vice versa);
    untagged ciphertexts pass"""
    for c in cts:
        lay = getattr(c, "layout", None)
        if lay is not None and not layout.same(lay):
            raise ValueError(f"ciphertext holds states in the {_describe(lay)} slot layout, "
                             f"this encoder / pipeline uses the {_describe(layout)} one")


def _describe(lay: SlotLayout) -> str:
    order = ", transposed bytes" if getattr(lay, "byte_order", "plain") == "transposed" else ""
    return f"{'periodic' if lay.periodic else 'reference'} (states={lay.states}{order})"


# the value decode's word types: name -> (bytes per word, signed, little-endian)
VALUE_DTYPES = {"u1": (1, False, True), "i1": (1, True, True), "<u2": (2, False, True), ">u2": (2, False, False),
                "<i2": (2, True, True), ">i2": (2, True, False)}


def value_dtype(dtype):
    """(width, signed, little) of a value dtype; ValueError for anything else.  32-bit words are refused on
    purpose: a word's error is its top byte's error times 256^(w - 1), so a 16-bit word is already good to ~13
    bits only and wider words would add no precision"""
    if dtype not in VALUE_DTYPES:
        raise ValueError(f"value dtype must be one of {sorted(VALUE_DTYPES)}, got {dtype!r} (words wider than 16 bits would add "
                         "no precision over 16: the top byte's error times 256^(w - 1) dominates)")
    return VALUE_DTYPES[dtype]


class ValueSlots:
    """StateEncoder.value_slots' result: weights / flags (G, slots) for the G = width groups, the per-slot
    constant (group constants rotated onto the word slot, plus the offset), and the rotation distance that
    brings group 1 onto group 0 (0 for 8-bit types)"""

    def __init__(self, dtype, weights, flags, const, distance):
        self.dtype, self.weights, self.flags, self.const, self.distance = dtype, weights, flags, const, distance

    @property
    def groups(self) -> int:
        return self.weights.shape[0]


class LinearSlots:
    """StateEncoder.linear_slots' result: weights / flags (G, slots) for the G kept cyclic diagonals of the matrix,
    the np.roll steps that bring each group onto its output slots, and two per-slot constants: `affine`, the map's
    own (the bias minus the zero point's share: sum_k roll(w_k * q_slots, steps[k]) + affine is y), and `const`,
    what the decode adds (affine plus the groups' E_0 terms rotated with them, as ValueSlots.const)"""

    def __init__(self, dtype, weights, flags, const, steps, diagonals, affine):
        self.dtype, self.weights, self.flags, self.const, self.steps, self.diagonals = dtype, weights, flags, const, steps, diagonals
        self.affine = affine

    @property
    def groups(self) -> int:
        return self.weights.shape[0]


# the tag of a byte-table value ciphertext (AESPipeline.transcipher_lut / to_lut): one real number
# per byte, but none of VALUE_DTYPES -- the slots hold table entries, not the integers the bytes spell
LUT_VALUE_TAG = "lut"


def tag_value_dtype(dtype, ct):
    """mark a value ciphertext with the dtype its slots hold (decode_values' default); returns it"""
    try:
        ct.value_dtype = dtype
    except AttributeError:  # a context whose ciphertexts carry no tag
        pass
    return ct


class StateEncoder:
    """pairs > 1: a multi-pair batch -- `pairs` independent ciphertext pairs,
    each holding `states` states in this layout, carried as ONE stacked hi and ONE stacked lo
    ciphertext (ctx.stack): encode takes (pairs, states, 16) / (pairs, 16) bytes, decode returns
    them, and every AES module runs on the stacks unchanged."""

    def __init__(self, ctx, states: int = 1, periodic: bool = False, pairs: int = 1, byte_order: str = "plain"):
        self.ctx = ctx
        self.sc = ctx.engine.slot_count
        self.layout = SlotLayout(self.sc, states, periodic)
        # byte_order="transposed" (AESPipeline(fips=True)): every clear byte state is transposed on its way in
        # (encode, nibble_slots, encode_packed) and out (decode, decode_packed), so callers see FIPS-197 byte order
        # while the ciphertexts hold T(state); the layout tag carries it
        if byte_order not in ("plain", "transposed"):
            raise ValueError(f"byte_order must be 'plain' or 'transposed', got {byte_order!r}")
        self.byte_order = self.layout.byte_order = byte_order
        self.stride = self.layout.unit  # rotation unit (REF: slot_count / 16)
        self.states = states
        if pairs < 1:
            raise ValueError("pairs must be >= 1")
        if pairs > 1 and getattr(ctx, "stack", None) is None:
            raise ValueError("multi-pair batches need a context with stacked ciphertexts (ctx.stack)")
        self.pairs = pairs
        # set by AESPipeline(true_fhe=True): renorm(hi, lo) -> hook(hi, lo), the bootstrap + snap
        # that replaces the secret-key renorm (zeta16_noise_reducer.BootstrapSnap)
        self.renorm_hook = None
        self.renorm_quad_hook = None  # true-FHE: two pairs per bootstrap (renorm_two)

    def _as_batch(self, state: np.ndarray) -> np.ndarray:
        """clear bytes in: the (B, 16) batch in the ciphertexts' byte order"""
        state = np.asarray(state, dtype=np.uint8)
        if state.shape == (16,) and self.states == 1:
            state = state[None, :]
        elif state.shape != (self.states, 16):
            raise ValueError(f"expected a ({self.states}, 16) uint8 state array, got {state.shape}")
        return self._order(state)

    def _order(self, state: np.ndarray) -> np.ndarray:
        """the byte transpose of a transposed encoder (an involution: in and out alike), else the state itself"""
        if self.byte_order != "transposed":
            return state
        from shift_columns import transpose_bytes
        return transpose_bytes(state)

    def _pack(self, nibbles: np.ndarray) -> np.ndarray:
        """nibbles (B, 16) -> slot vector; slot i*unit + b <- zeta^nibbles[b, i] (periodic: tiled)"""
        grid = np.ones((16, self.stride), dtype=np.complex128)
        grid[:, :nibbles.shape[0]] = ZetaEncoder.to_zeta(nibbles.astype(np.uint8).T, 16)
        return self.layout.tile(grid.reshape(-1))

    def nibble_slots(self, state: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(hi, lo): the uint8 nibble of every slot for a PUBLIC byte state in this encoder's layout -- what
        _pack encodes, before the Zeta16 map: to_zeta(nibble_slots(s)[k]) equals the packed slot vector slot
        for slot (slots that hold no state carry nibble 0 = the 1 + 0j _pack fills them with).  The public
        operand of AddRoundKey.public / Engine.lut_eval_public."""
        if self.pairs > 1:
            raise ValueError("nibble_slots: public operands of multi-pair batches (pairs > 1) are not supported")
        st = self._as_batch(state)

        def slots(nib):
            grid = np.zeros((16, self.stride), dtype=np.uint8)
            grid[:, :nib.shape[0]] = nib.T
            return np.ascontiguousarray(self.layout.tile(grid.reshape(-1)))

        return slots(st >> 4), slots(st & 0x0F)

    def _take(self, slots: np.ndarray) -> np.ndarray:
        """slot vector -> (B, 16) state slots"""
        return slots[:16 * self.stride].reshape(16, self.stride)[:, :self.states].T

    def _pair_states(self, state: np.ndarray):
        """(pairs, ...) bytes -> the per-pair state arrays; a single pair's shape broadcasts"""
        state = np.asarray(state, dtype=np.uint8)
        one = (16,) if self.states == 1 else (self.states, 16)
        if state.shape == one:
            return [state] * self.pairs
        if state.shape != (self.pairs,) + one:
            raise ValueError(f"expected a {(self.pairs,) + one} uint8 state array, got {state.shape}")
        return list(state)

    def encode(self, state: np.ndarray, seeded: bool = False) -> Tuple[Any, Any]:
        """seeded=True: the pair is made by one batched seeded symmetric encryption
        (ctx.encrypt_seeded_many) and travels through dump_ct_seeded as b rows plus ids; pairs > 1 is refused, a
        stack being an operation's result"""
        if seeded:
            if self.pairs > 1:
                raise ValueError("encode: seeded encryption of multi-pair batches (pairs > 1) is not supported")
            if getattr(self.ctx, "encrypt_seeded_many", None) is None:
                raise ValueError("encode: seeded encryption needs a context with encrypt_seeded_many (engine_context.EngineContext)")
            st = self._as_batch(self._pair_states(state)[0])
            return tag_layout(self.layout, *self.ctx.encrypt_seeded_many([self._pack(st >> 4), self._pack(st & 0x0F)]))
        if self.pairs > 1:
            his, los = zip(*[self._encode1(s) for s in self._pair_states(state)])
            return tag_layout(self.layout, self.ctx.stack(his), self.ctx.stack(los))
        return self._encode1(self._pair_states(state)[0])

    def encode_many(self, states, seeded: bool = False):
        """[(hi, lo)] of several states; seeded=True: ONE batched seeded encryption for all of them (the 22
        ciphertexts of 11 round keys), consecutive seed ids in (state, hi / lo) order"""
        if not seeded:
            return [self.encode(s) for s in states]
        if self.pairs > 1:
            raise ValueError("encode_many: seeded encryption of multi-pair batches (pairs > 1) is not supported")
        vecs = []
        for s in states:
            st = self._as_batch(self._pair_states(s)[0])
            vecs += [self._pack(st >> 4), self._pack(st & 0x0F)]
        cts = tag_layout(self.layout, *self.ctx.encrypt_seeded_many(vecs))
        return [(cts[2 * i], cts[2 * i + 1]) for i in range(len(cts) // 2)]

    def _encode1(self, state):
        st = self._as_batch(state)
        return tag_layout(self.layout, self.ctx.encrypt(self._pack(st >> 4)), self.ctx.encrypt(self._pack(st & 0x0F)))

    def decode(self, ct_hi, ct_lo) -> np.ndarray:
        check_layout(self.layout, ct_hi, ct_lo)
        if self.pairs > 1:
            return np.stack([self._decode1(h, l) for h, l in zip(self.ctx.unstack(ct_hi), self.ctx.unstack(ct_lo))])
        return self._decode1(ct_hi, ct_lo)

    def _decode1(self, ct_hi, ct_lo) -> np.ndarray:
        hi = ZetaEncoder.from_zeta(self._take(self.ctx.decrypt(ct_hi)), 16)
        lo = ZetaEncoder.from_zeta(self._take(self.ctx.decrypt(ct_lo)), 16)
        out = self._order(((hi << 4) | lo).astype(np.uint8))
        return out[0] if self.states == 1 else out

    def _float_slots(self, per_byte: np.ndarray) -> np.ndarray:
        """(states, 16) floats in the caller's byte order -> the slot vector with each number in its byte's slot
        and 0 in every slot that holds no state (nibble_slots' placement, on floats)"""
        v = np.asarray(per_byte, np.float64).reshape(self.states, 16)
        if self.byte_order == "transposed":  # shift_columns.transpose_bytes' map, on floats
            v = np.swapaxes(v.reshape(-1, 4, 4), -1, -2).reshape(v.shape)
        grid = np.zeros((16, self.stride), np.float64)
        grid[:, :self.states] = v.T
        return np.ascontiguousarray(self.layout.tile(grid.reshape(-1)))

    @property
    def word_distance(self) -> int:
        """the slot distance between bytes 2k and 2k + 1 of a block in this layout and byte order: the rotation
        that brings a 16-bit word's second byte onto its first (unit in the plain order, 4 unit transposed)"""
        at = self._order(np.arange(16, dtype=np.uint8)[None, :])[0].astype(np.int64)  # an involution: where byte i sits
        d = {int(at[2 * k + 1] - at[2 * k]) for k in range(8)}
        assert len(d) == 1 and min(d) > 0
        return d.pop() * self.stride

    def value_slots(self, spec) -> "ValueSlots":
        """spec = (dtype, gain, offset): the per-slot weights, flags and constant with which the value decode
        (xor_value_lut.TypedValueLUT) leaves gain * q + offset in the slot of each word's first
        byte, q the integer the word's bytes spell in `dtype`, and 0 in every other slot.  dtype: one of
        VALUE_DTYPES; gain, offset: scalars or arrays broadcastable to (16 // w,) or (states, 16 // w), w the
        word's width in bytes (gain None: 256^-w).  Group g weighs byte g of every word by gain * 256^(its
        significance); the top byte of a signed type carries flag 1 (signed hi nibble)."""
        dtype, gain, offset = spec
        w, signed, little = value_dtype(dtype)
        nw = 16 // w
        try:
            g = np.broadcast_to(np.asarray(256.0 ** -w if gain is None else gain, np.float64), (self.states, nw))
            off = np.broadcast_to(np.asarray(offset, np.float64), (self.states, nw))
        except ValueError:
            raise ValueError(f"value_slots: gain and offset must broadcast to ({nw},) or ({self.states}, {nw}) for dtype {dtype!r}") from None
        if not (np.all(np.isfinite(g)) and np.all(np.isfinite(off))):
            raise ValueError("value_slots: gain and offset must be finite")
        weights, flags = np.zeros((w, self.sc)), np.zeros((w, self.sc), np.uint8)
        const = np.zeros(self.sc)
        first = np.zeros((self.states, 16))
        first[:, ::w] = off
        const += self._float_slots(first)  # the offset sits with the word: the slot of its first byte
        for j in range(w):  # group j: byte j of every word
            sig = j if little else w - 1 - j
            top = signed and sig == w - 1
            wb, fb = np.zeros((self.states, 16)), np.zeros((self.states, 16))
            wb[:, j::w] = g * 256.0 ** sig
            fb[:, j::w] = 1.0 if top else 0.0
            weights[j] = self._float_slots(wb)
            flags[j] = self._float_slots(fb).astype(np.uint8)
            # E_0 of both nibbles: 16 * 7.5 + 7.5, the signed hi nibble's E_0 is -0.5; rotated with its group
            const += np.roll(weights[j] * (16.0 * (-0.5 if top else 7.5) + 7.5), -j * self.word_distance)
        return ValueSlots(dtype, weights, flags, const, self.word_distance if w > 1 else 0)

    def _position_slots(self, per_position: np.ndarray) -> np.ndarray:
        """(states, 16) floats indexed by SLOT POSITION (position p of state b: slot p * unit + b) -> the slot vector,
        0 in every slot that holds no state: _float_slots without the byte order"""
        grid = np.zeros((16, self.stride), np.float64)
        grid[:, :self.states] = np.asarray(per_position, np.float64).reshape(self.states, 16).T
        return np.ascontiguousarray(self.layout.tile(grid.reshape(-1)))

    def linear_slots(self, W, bias=0.0, dtype: str = "i1", in_scale=None, zero_point=0.0) -> "LinearSlots":
        """The weight groups with which the value decode applies a 16 x 16 matrix to the decoded bytes of every state
        (xor_value_lut.LinearValueLUT): output byte position i of state b holds
            y[b, i] = sum_j W[b, i, j] * (q[b, j] - zero_point[j]) * in_scale + bias[b, i],
        q the block's bytes read as `dtype` ("u1" or "i1").  W: (16, 16) or (states, 16, 16); bias broadcasts to
        (states, 16); in_scale a scalar (None: 1/256); zero_point a scalar or (16,).

        The diagonal method in slot-position space.  Position p holds byte at[p] (the encoder's own byte map, so the
        transposed order works), W'[po, pi] = W[at[po], at[pi]], and group k weighs position p's slot by
        W'[(p - k) % 16, p] * in_scale: what sits at p belongs to output position p - k, so the group is rolled by
        steps[k] = -k * unit (slot j takes slot j + k unit; the state is 16-unit-periodic, so that is cyclic inside
        each state).  sum_k roll(X_k, steps[k]) + affine is y.  A diagonal that is zero in every state is dropped
        (`diagonals` lists the kept k); "i1" flags every state slot (signed hi nibble), as value_slots does."""
        if self.pairs > 1:
            raise ValueError("linear_slots: multi-pair batches (pairs > 1) are not supported")
        w, signed, _ = value_dtype(dtype)
        if w != 1:
            raise ValueError(f"linear_slots: the matrix acts on bytes, dtype must be 'u1' or 'i1', got {dtype!r}")
        W = np.asarray(W, np.float64)
        if W.shape not in ((16, 16), (self.states, 16, 16)):
            raise ValueError(f"linear_slots: W must be (16, 16) or ({self.states}, 16, 16), got {W.shape}")
        W = np.broadcast_to(W, (self.states, 16, 16))
        scale = 1.0 / 256.0 if in_scale is None else float(in_scale)
        try:
            b = np.broadcast_to(np.asarray(bias, np.float64), (self.states, 16))
            zp = np.broadcast_to(np.asarray(zero_point, np.float64), (16,))
        except ValueError:
            raise ValueError(f"linear_slots: bias must broadcast to ({self.states}, 16) and zero_point to (16,)") from None
        if not (np.all(np.isfinite(W)) and np.all(np.isfinite(b)) and np.all(np.isfinite(zp)) and np.isfinite(scale)):
            raise ValueError("linear_slots: W, bias, zero_point and in_scale must be finite")
        at = self._order(np.arange(16, dtype=np.uint8)[None, :])[0].astype(np.int64)  # the byte at slot position p
        Wp = W[:, at][:, :, at]
        p = np.arange(16)
        diag = [Wp[:, (p - k) % 16, p] * scale for k in range(16)]  # (states, 16) per diagonal, by input position
        keep = [k for k in range(16) if np.any(diag[k])] or [0]
        weights = np.stack([self._position_slots(diag[k]) for k in keep])
        state_slots = self._position_slots(np.ones((self.states, 16)))
        flags = np.tile(state_slots.astype(np.uint8) if signed else np.zeros(self.sc, np.uint8), (len(keep), 1))
        steps = [-k * self.stride for k in keep]
        e0 = 16.0 * (-0.5 if signed else 7.5) + 7.5  # E_0 of both nibbles, as value_slots
        affine = self._float_slots(b - scale * (W @ zp))
        const = affine.copy()
        for wk, st in zip(weights, steps):
            const += np.roll(wk * e0, st)
        return LinearSlots(dtype, np.ascontiguousarray(weights), np.ascontiguousarray(flags), const, steps, keep, affine)

    def lut_slots(self, gain=1.0, c00: float = 0.0):
        """(weights, const): the per-slot weight and constant vectors of the byte-table decode
        (xor_value_lut.ByteValueLUT) -- gain (a scalar, or broadcastable to (16,) or (states, 16), in
        the caller's byte order) in the slot of each byte and 0 in every slot that holds no state, and
        const = weights * c00 (the table's mean, byte_value_table's C_00).  _float_slots places the numbers, so the
        transposed byte order works"""
        if self.pairs > 1:
            raise ValueError("lut_slots: multi-pair batches (pairs > 1) are not supported")
        try:
            g = np.broadcast_to(np.asarray(gain, np.float64), (self.states, 16))
        except ValueError:
            raise ValueError(f"lut_slots: gain must broadcast to (16,) or ({self.states}, 16)") from None
        if not (np.all(np.isfinite(g)) and np.isfinite(c00)):
            raise ValueError("lut_slots: gain must be finite")
        weights = self._float_slots(g)
        return weights, weights * float(c00)

    def lut_bank_slots(self, select, gain=1.0, c00s=(0.0,)):
        """(sel, weights, const): lut_slots for a BANK of byte tables (xor_value_lut.ByteValueBank).
        select: the table of each byte -- integers in [0, T), T = len(c00s), broadcastable to (16,) or (states, 16) in
        the caller's byte order; sel: uint8 per slot, the slot's table index and 0 in every slot that holds no state;
        weights as lut_slots'; const = weights * c00s[sel] (each slot's own table's mean).  _float_slots places the
        indices as it places the gains, so both layouts and the transposed byte order work"""
        if self.pairs > 1:
            raise ValueError("lut_bank_slots: multi-pair batches (pairs > 1) are not supported")
        c = np.asarray(c00s, np.float64)
        if c.ndim != 1 or not 1 <= c.size <= 256 or not np.all(np.isfinite(c)):
            raise ValueError("lut_bank_slots: c00s must be 1..256 finite reals, one per table")
        s = np.asarray(select)
        if s.dtype == bool or not np.issubdtype(s.dtype, np.integer):
            raise ValueError(f"lut_bank_slots: select must be integers (table indices), got dtype {s.dtype}")
        try:
            s = np.broadcast_to(s, (self.states, 16))
        except ValueError:
            raise ValueError(f"lut_bank_slots: select must broadcast to (16,) or ({self.states}, 16)") from None
        if s.min() < 0 or s.max() >= c.size:
            raise ValueError(f"lut_bank_slots: select must lie in [0, {c.size})")
        weights = self.lut_slots(gain)[0]
        sel = np.ascontiguousarray(self._float_slots(s.astype(np.float64)).astype(np.uint8))
        return sel, weights, weights * c[sel]

    def values_from_slots(self, slots: np.ndarray, dtype=None) -> np.ndarray:
        """the pure unpacking of decode_values: a slot vector whose word slots hold one real number per word
        (xor_value_lut's output) -> the (states, 16 // w) float array in the caller's byte order, (16 // w,) for one
        state -- _pack's slot order and the encoder's byte order undone, imaginary parts dropped.  dtype None: bytes"""
        w = 1 if dtype == LUT_VALUE_TAG else value_dtype("u1" if dtype is None else dtype)[0]
        slots = np.asarray(slots)
        if slots.shape != (self.sc,):
            raise ValueError(f"expected a slot vector of {self.sc} entries, got shape {slots.shape}")
        v = np.ascontiguousarray(self._take(slots.real.astype(np.float64)))
        if self.byte_order == "transposed":  # shift_columns.transpose_bytes' map, on floats
            v = np.ascontiguousarray(np.swapaxes(v.reshape(-1, 4, 4), -1, -2)).reshape(v.shape)
        if w > 1:
            v = np.ascontiguousarray(v[:, ::w])  # a word sits in the slot of its first byte
        return v[0] if self.states == 1 else v

    def decode_values(self, ct, dtype=None) -> np.ndarray:
        """client side: decrypt a value ciphertext (AESPipeline.transcipher_values / to_values) into the
        (states, 16 // w) float array of gain * q + offset, (16 // w,) for one state.  The ciphertext carries the
        dtype it was made with (tag_value_dtype): that is the default, and a contradicting `dtype` is refused"""
        if self.pairs > 1:
            raise ValueError("decode_values: multi-pair batches (pairs > 1) are not supported")
        check_layout(self.layout, ct)
        tag = getattr(ct, "value_dtype", None)
        if dtype is not None and tag is not None and dtype != tag:
            raise ValueError(f"decode_values: the ciphertext holds {tag!r} values, asked for {dtype!r}")
        return self.values_from_slots(self.ctx.decrypt(ct), dtype if dtype is not None else tag)

    # ---------------------------------------------------------------- packed form
    PACK_DEPTH = 1  # pack(): one plaintext product

    def pack(self, ct_hi, ct_lo):
        """(hi, lo) -> ONE ciphertext, hi on the first half of every 2P-slot block and lo on the
        second: hi * mask_0 + lo * mask_1 (one level; both halves are P-periodic, so no rotation)"""
        if not self.layout.packable:
            raise ValueError("the packed form needs the periodic layout with 2 * period <= slot count")
        if isinstance(ct_hi, ConjSum) or isinstance(ct_lo, ConjSum):
            # the masks are real: pack(conj a, conj b) = conj(pack(a, b)), so a pair of
            # utils.ConjSum packs into one (both halves' S1 packed, and both S2)
            if not (isinstance(ct_hi, ConjSum) and isinstance(ct_lo, ConjSum)):
                return self.pack(conj_sum(self.ctx, ct_hi), conj_sum(self.ctx, ct_lo))
            return ConjSum(self.pack(ct_hi.s1, ct_lo.s1), self.pack(ct_hi.s2, ct_lo.s2))
        ctx = self.ctx
        if getattr(self, "_half_pts", None) is None:
            self._half_pts = [ctx.encode(self.layout.half_mask(w)) for w in (0, 1)]
        return ctx.add(ctx.multiply(ct_hi, self._half_pts[0]), ctx.multiply(ct_lo, self._half_pts[1]))

    def _packed_slots(self, st: np.ndarray) -> np.ndarray:
        hi, lo = self._pack(st >> 4), self._pack(st & 0x0F)
        return np.where(self.layout.half_mask(0).real > 0.5, hi, lo)

    def encode_packed(self, state: np.ndarray):
        """a state (batch) encrypted directly in the packed form"""
        if self.pairs > 1:
            cts = [self.ctx.encrypt(self._packed_slots(self._as_batch(s))) for s in self._pair_states(state)]
            return tag_layout(self.layout, self.ctx.stack(cts))[0]
        return tag_layout(self.layout, self.ctx.encrypt(self._packed_slots(self._as_batch(self._pair_states(state)[0]))))[0]

    def decode_slots(self, hi_slots: np.ndarray, lo_slots: np.ndarray) -> np.ndarray:
        """_decode1 on slot vectors: the (hi, lo) Zeta16 slot vectors of one pair (decrypted elsewhere, a result pack's
        members above all) -> the (states, 16) bytes in the caller's byte order, (16,) for one state"""
        if self.pairs > 1:
            raise ValueError("decode_slots: multi-pair batches (pairs > 1) are not supported")
        hs, ls = np.asarray(hi_slots), np.asarray(lo_slots)
        if hs.shape != (self.sc,) or ls.shape != (self.sc,):
            raise ValueError(f"expected two slot vectors of {self.sc} entries, got shapes {hs.shape} and {ls.shape}")
        hi = ZetaEncoder.from_zeta(self._take(hs), 16)
        lo = ZetaEncoder.from_zeta(self._take(ls), 16)
        out = self._order(((hi << 4) | lo).astype(np.uint8))
        return out[0] if self.states == 1 else out

    def _check_pack_meta(self, meta) -> None:
        """a result pack's meta against this encoder: one pair per ciphertext, the periodic layout, the same slot count,
        and every member's layout tag this encoder's own"""
        if self.pairs > 1:
            raise ValueError("decode_packed: result packs of multi-pair batches (pairs > 1) are not supported")
        if not self.layout.periodic:
            raise ValueError("decode_packed: a result pack holds periodic results; this encoder uses the reference layout")
        if int(meta["slots"]) != self.sc:
            raise ValueError(f"decode_packed: the pack was made for {meta['slots']} slots, this encoder has {self.sc}")
        if int(meta["period"]) % self.layout.period:
            raise ValueError(f"decode_packed: the pack's period {meta['period']} is no multiple of this layout's {self.layout.period}")
        for tag in meta["layouts"]:
            if tag is not None and not self.layout.same(_layout_of_tag(tag)):
                raise ValueError(f"decode_packed: a member holds states in the {_describe(_layout_of_tag(tag))} slot layout, "
                                 f"this encoder uses the {_describe(self.layout)} one")

    def _decode_members(self, slots, meta) -> list:
        """decode_packed(array, meta) after the decryption: `slots` are the members' slot vectors in member order
        (result_pack.unpack_results / split_slots)"""
        tags = list(meta["value_dtypes"])
        present = list(meta.get("present", [True] * len(tags)))
        if len(slots) != len(tags):
            raise ValueError(f"decode_packed: {len(slots)} slot vectors for {len(tags)} members")
        if not all(present):
            raise ValueError("decode_packed: the pack has an absent member; decode its members with decode_slots / values_from_slots")
        out, j = [], 0
        while j < len(tags):
            if tags[j] is not None:
                out.append(self.values_from_slots(slots[j], tags[j]))
                j += 1
                continue
            if j + 1 >= len(tags) or tags[j + 1] is not None:
                raise ValueError(f"decode_packed: an odd run of untagged members ends at member {j}: (hi, lo) pairs come two at a time")
            out.append(self.decode_slots(slots[j], slots[j + 1]))
            j += 2
        return out

    def decode_packed(self, ct, meta=None):
        """decode_packed(ct): the packed hi | lo form of DESIGN.md §4c, as ever.  decode_packed(array, meta): a RESULT
        PACK (result_pack.dump_results) -- the client's one decryption, then one entry per result in
        member order: a member tagged as a value ciphertext is its float array (values_from_slots under its tag),
        consecutive untagged members are taken two at a time as (hi, lo) and give the pair's bytes (one entry per
        pair); an odd run of untagged members, an absent member, pairs > 1, the reference layout and a meta of
        another slot count or layout raise ValueError.  A meta with "ring" (dump_results(..., ring=))
        names a ring-switched pack: the (2, 2, ring) array is decrypted in the small ring, in numpy, under the subring
        secret (unpack_results), and decoded the same way"""
        if meta is not None:
            from result_pack import unpack_results
            self._check_pack_meta(meta)
            return self._decode_members(unpack_results(self.ctx, ct, meta), meta)
        check_layout(self.layout, ct)
        if self.pairs > 1:
            return np.stack([self._decode_packed1(c) for c in self.ctx.unstack(ct)])
        return self._decode_packed1(ct)

    def _decode_packed1(self, ct) -> np.ndarray:
        z = self.ctx.decrypt(ct)
        hi = ZetaEncoder.from_zeta(self._take(z), 16)
        lo = ZetaEncoder.from_zeta(self._take(z[self.layout.period:]), 16)
        out = self._order(((hi << 4) | lo).astype(np.uint8))
        return out[0] if self.states == 1 else out

    UNPACK_DEPTH = 1  # unpack(): one mask product after the rotation

    def _fold_conj(self, *cts):
        """the renorm's inputs with any utils.ConjSum summed homomorphically unless the conjugation
        fold is on (FOLDS.conj; strict renorms are the identity on the message)"""
        return tuple(c if FOLDS.conj else conj_sum(self.ctx, c) for c in cts)

    def unpack(self, ct, z=None):
        """the packed state -> its (hi, lo) pair, homomorphically (the inverse of pack): both halves
        are P-periodic inside the 2P-periodic message, so z = rot_P(ct) holds lo where ct holds hi
        and vice versa, and hi = z + m0 (ct - z), lo = ct - m0 (ct - z) -- one rotation and one
        mask product (UNPACK_DEPTH levels), every slot of both outputs as the packed input's.
        z: rot_P(ct) when the caller has it (from a hoisted key switch)"""
        ctx = self.ctx
        if getattr(self, "_half_pts", None) is None:
            self._half_pts = [ctx.encode(self.layout.half_mask(w)) for w in (0, 1)]
        if z is None:
            z = ctx.rotate(ct, self.layout.period)
        t = ctx.multiply(ctx.sub(ct, z), self._half_pts[0])
        return tag_layout(self.layout, ctx.add(z, t), ctx.sub(ct, t))

    def renorm_packed(self, ct, level=None):
        """renorm of a packed state, packed again (ct may be a utils.ConjSum: s1 + conj(s2) renormalised
        with the conjugation folded into the decryption when FOLDS.conj)"""
        (ct,) = self._fold_conj(ct)
        lv = None if _RENORM_FRESH else level
        single = self.ctx.renorm_single
        if isinstance(ct, ConjSum):
            if takes_kw(single, "period", "conj"):
                tally_renorm(self.ctx, ct.s1)
                return single(ct.s1, lv, period=2 * self.layout.period, conj=ct.s2)
            ct = conj_sum(self.ctx, ct)
        tally_renorm(self.ctx, ct)
        if takes_kw(single, "period"):
            return single(ct, lv, period=2 * self.layout.period)
        return single(ct, lv)  # a context whose renorm_single takes no period

    def renorm_perm(self, ct_hi, ct_lo, perm, level=None):
        """renorm(hi, lo) followed by a byte permutation (output byte i <- input byte perm[i]), the
        permutation folded into the device renorm (aesfhe_renorm_periodic_perm; FOLDS.sr, the caller
        checks renorm_perm_ok first).  utils.ConjSum halves are folded as in renorm"""
        if not FOLDS.sr:
            raise RuntimeError("renorm_perm: the ShiftRows fold is off (utils.FOLDS.sr)")
        ct_hi, ct_lo = self._fold_conj(ct_hi, ct_lo)
        conj = None
        if isinstance(ct_hi, ConjSum) and isinstance(ct_lo, ConjSum):
            conj, ct_hi, ct_lo = (ct_hi.s2, ct_lo.s2), ct_hi.s1, ct_lo.s1
        else:
            ct_hi, ct_lo = conj_sum(self.ctx, ct_hi), conj_sum(self.ctx, ct_lo)
        check_layout(self.layout, ct_hi, ct_lo)
        tally_renorm(self.ctx, ct_hi, ct_lo)
        return tag_layout(self.layout, *self.ctx.renorm_periodic_perm(ct_hi, ct_lo, self.layout.period, perm,
                                                                      None if _RENORM_FRESH else level, conj=conj))

    def renorm_unpack_perm(self, ct, perm, level=None):
        """renorm_unpack followed by a byte permutation of both halves, folded into the device renorm
        (aesfhe_renorm_unpack_perm; FOLDS.sr and FOLDS.unpack); the caller checks renorm_perm_ok"""
        if not (FOLDS.sr and FOLDS.unpack):
            raise RuntimeError("renorm_unpack_perm: the ShiftRows / unpack folds are off (utils.FOLDS)")
        (ct,) = self._fold_conj(ct)
        conj = None
        if isinstance(ct, ConjSum):
            conj, ct = ct.s2, ct.s1
        check_layout(self.layout, ct)
        tally_renorm(self.ctx, ct)
        return tag_layout(self.layout, *self.ctx.renorm_unpack_perm(ct, self.layout.period, perm, None if _RENORM_FRESH else level,
                                                                    conj=conj))

    def renorm_perm_ok(self, ct=None) -> bool:
        """whether renorm_perm / renorm_unpack_perm run on this encoder / context (the ShiftRows and
        unpack folds on, one period-16 state pair on the device, the engine's direct period-32 codec)"""
        if not (FOLDS.sr and FOLDS.unpack):
            return False
        if not (getattr(self.ctx, "renorm_periodic_perm", None) is not None and getattr(self.ctx, "renorm_unpack_perm", None) is not None
                and self.pack_renorm_direct(ct, need_pack=False)):
            return False
        direct = getattr(getattr(self.ctx, "engine", None), "direct32", None)
        return direct is None or bool(direct())

    def pack_renorm_direct(self, ct=None, need_pack: bool = True) -> bool:
        """whether renorm_pack runs as the device's packing renorm (FOLDS.pack; then its inputs need no
        pack level); ct: an input of the pair -- a stack of several state pairs takes pack + renorm"""
        if not ((FOLDS.pack or not need_pack) and getattr(self.ctx, "renorm_pack", None) is not None and self.renorm_hook is None
                and self.layout.periodic and self.layout.period == 16 and self.pairs == 1):
            return False
        members = getattr(getattr(self.ctx, "engine", None), "members", None)
        return ct is None or members is None or members(ct.s1 if isinstance(ct, ConjSum) else ct) == 1

    def renorm_pack(self, ct_hi, ct_lo, level=None):
        """renorm_packed(pack(hi, lo)): with the pack fold (FOLDS.pack) and one period-16 state pair the
        device renorm encodes the snapped pair straight into the packed form (aesfhe_renorm_pack: no mask
        products, no pack level; utils.ConjSum halves folded as in renorm); otherwise pack, then renorm"""
        if self.pack_renorm_direct(ct_hi):
            ct_hi, ct_lo = self._fold_conj(ct_hi, ct_lo)
            rp = self.ctx.renorm_pack
            conj = None
            if isinstance(ct_hi, ConjSum) and isinstance(ct_lo, ConjSum):
                conj, ct_hi, ct_lo = (ct_hi.s2, ct_lo.s2), ct_hi.s1, ct_lo.s1
            else:
                ct_hi, ct_lo = conj_sum(self.ctx, ct_hi), conj_sum(self.ctx, ct_lo)
            check_layout(self.layout, ct_hi, ct_lo)
            tally_renorm(self.ctx, ct_hi, ct_lo)
            return tag_layout(self.layout, rp(ct_hi, ct_lo, self.layout.period, None if _RENORM_FRESH else level, conj=conj))[0]
        return self.renorm_packed(self.pack(ct_hi, ct_lo), level)

    def renorm_unpack(self, ct, level=None) -> Tuple[Any, Any]:
        """renorm of a packed state into the (hi, lo) pair at `level`.  Strict (FOLDS.unpack off): the
        packed renorm at level + UNPACK_DEPTH, then the homomorphic unpack; with the fold the device
        renorm's encoder gathers the two halves (aesfhe_renorm_unpack).  ct may be a utils.ConjSum"""
        if not FOLDS.unpack or getattr(self.ctx, "renorm_unpack", None) is None:
            lv = None if level is None else level + self.UNPACK_DEPTH
            return self.unpack(self.renorm_packed(ct, lv))
        (ct,) = self._fold_conj(ct)
        lv = None if _RENORM_FRESH else level
        if isinstance(ct, ConjSum):
            check_layout(self.layout, ct.s1)
            tally_renorm(self.ctx, ct.s1)
            return tag_layout(self.layout, *self.ctx.renorm_unpack(ct.s1, self.layout.period, lv, conj=ct.s2))
        check_layout(self.layout, ct)
        tally_renorm(self.ctx, ct)
        return tag_layout(self.layout, *self.ctx.renorm_unpack(ct, self.layout.period, lv))

    def renorm(self, ct_hi, ct_lo, level=None) -> Tuple[Any, Any]:
        """decode -> re-encode (REF/pipeline.py:65-69), done on the device when available;
        `level`: the level the next step needs (None = fresh), honoured by the device path.
        With a renorm_hook (true-FHE mode) the hook runs instead (it reads `level` as the next step's need).
        hi / lo may be utils.ConjSum (s1 + conj(s2)): the periodic device renorm folds the conjugation
        into its decryption; any other path sums them first."""
        ct_hi, ct_lo = self._fold_conj(ct_hi, ct_lo)
        if isinstance(ct_hi, ConjSum) or isinstance(ct_lo, ConjSum):
            per = getattr(self.ctx, "renorm_periodic", None)
            if (isinstance(ct_hi, ConjSum) and isinstance(ct_lo, ConjSum) and self.renorm_hook is None and self.layout.periodic
                    and per is not None and takes_kw(per, "conj")):
                check_layout(self.layout, ct_hi.s1, ct_lo.s1)
                tally_renorm(self.ctx, ct_hi.s1, ct_lo.s1)
                return tag_layout(self.layout, *per(ct_hi.s1, ct_lo.s1, self.layout.period, None if _RENORM_FRESH else level,
                                                    conj=(ct_hi.s2, ct_lo.s2)))
            ct_hi, ct_lo = conj_sum(self.ctx, ct_hi), conj_sum(self.ctx, ct_lo)
        check_layout(self.layout, ct_hi, ct_lo)
        if self.renorm_hook is None:
            tally_renorm(self.ctx, ct_hi, ct_lo)
        return tag_layout(self.layout, *self._renorm(ct_hi, ct_lo, level))

    def renorm_two(self, p, q, level=None):
        """renorm of two (hi, lo) pairs at one point of a step: in true-FHE mode with a quad hook
        (zeta16_noise_reducer.BootstrapSnap.apply_quad) ONE bootstrap refreshes all four
        ciphertexts; otherwise two renorm calls"""
        if self.renorm_quad_hook is not None:
            ps, qs = self._fold_conj(*p), self._fold_conj(*q)
            if not any(isinstance(c, ConjSum) for c in ps + qs):
                check_layout(self.layout, *ps, *qs)
                a, b = self.renorm_quad_hook(ps, qs, level)
                return tag_layout(self.layout, *a), tag_layout(self.layout, *b)
        return self.renorm(*p, level), self.renorm(*q, level)

    def _renorm(self, ct_hi, ct_lo, level):
        if self.renorm_hook is not None:
            return self.renorm_hook(ct_hi, ct_lo, level)
        per = getattr(self.ctx, "renorm_periodic", None)
        if self.layout.periodic and per is not None:
            return per(ct_hi, ct_lo, self.layout.period, None if _RENORM_FRESH else level)
        fast = getattr(self.ctx, "renorm_pair", None)
        if fast is not None:
            st = self.layout.renorm_states
            if level is not None and not _RENORM_FRESH:
                return fast(ct_hi, ct_lo, states=st, level=level)
            return fast(ct_hi, ct_lo) if st == 1 else fast(ct_hi, ct_lo, states=st)
        return self.encode(self.decode(ct_hi, ct_lo))
