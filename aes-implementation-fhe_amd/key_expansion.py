"""Homomorphic AES key schedule: the 11 round keys from ONE encrypted 16-byte key (AES-128), or the
15 round keys from an encrypted 32-byte key (AES-256).  AES-192's six-word stride straddles the
16-byte state and is not expanded here: its 13 round keys come from the client (EncryptedRoundKeys.from_pairs).

One 128-bit schedule step maps the words w0..w3 of round key r - 1 to
    w_j' = w0 ^ ... ^ w_j ^ SubWord(RotWord(w3)) ^ rcon_r,   j = 0..3
(FIPS-197 §5.2 unrolled: w_j' = w_{j-1}' ^ w_j).  Written with no step serial over the words:

  prefix   x' = x ^ rcon_r (a PUBLIC operand on row 0 of word 0: AddRoundKey.public), then the prefix XOR over the
           words in two doubling steps, y = x' ^ shift1(x'), P = y ^ shift2(y); shift_k moves every word k words up
           and fills the vacated words with the codeword of nibble 0 (1 + 0j in the Zeta16 code, not 0).  Every
           prefix holds rcon_r exactly once.
  sub      SubBytes of the whole key (byte-wise, so it runs before the broadcast and independently of the prefix
           branch), then ONE masked rotation sum that rotates word 3 by one byte and copies it into all four words.
  out      XOR4 of the two branches.  A renorm follows every LUT step, as everywhere else in the pipeline.

Every move is a rotation by a multiple of layout.unit under SlotLayout.cell_mask masks, built the way
shift_columns.apply_terms builds its terms, and evaluated by ctx.rot_pt_affine (the engine's aesfhe_rot_pt_affine:
the masked rotation sum plus a fill plaintext, one kernel).  Words are the columns of the FIPS byte order: with
byte_order "plain" slot position r + 4c holds row r of word c, with "transposed" (AESPipeline(fips=True)) it holds
row c of word r; SchedulePlan takes the order and produces the offsets and masks of both.  The state being
16-unit-periodic (ShiftRows' rotations rely on the same), offsets are taken mod 16 positions: the broadcast's 8
(row, word) offset classes are 4 rotations.

The 256-bit schedule (FIPS-197 §5.2, Nk = 8) is the same three pieces on two round keys.  With K_0, K_1 the halves of
the key and r = 2..14:
    r even:  K_r = prefix(K_{r-2} ^ RCON[r // 2 - 1]) ^ broadcast(SubBytes(K_{r-1}))
    r odd:   K_r = prefix(K_{r-2})                    ^ wordcopy(SubBytes(K_{r-1}))
wordcopy is the broadcast without RotWord: row rho of every word takes row rho of word 3 (4 rotations again, one of
them the identity: word 3 keeps itself).  An odd step has no constant, hence no public XOR and no renorm after it.

``schedule_step_slots`` / ``schedule_step_slots256`` are the numpy models of the plan on nibble slot vectors (no
engine), ``schedule_step_bytes`` / ``schedule_step_bytes256`` the byte models of the debug stages; ``KeyExpansion`` runs it on
an AESPipeline's own modules; ``EncryptedRoundKeys`` is what every pipeline method takes in place of clear round keys.
No reference counterpart (REF/test/test_aes_pipeline_roundtrip.py:20-48 expands the key in clear).
"""
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from aes_keyschedule import RCON, SBOX
from state_encoder import check_layout, tag_layout
from utils import NEED_SR_ARK, NEED_XOR, drop_to


def word_pos(row: int, word: int, byte_order: str = "plain") -> int:
    """slot position (in units) of row `row` of word `word`"""
    if byte_order == "plain":
        return row + 4 * word
    if byte_order == "transposed":
        return word + 4 * row
    raise ValueError(f"byte_order must be 'plain' or 'transposed', got {byte_order!r}")


def _centered(d: int) -> int:
    """the offset d mod 16 positions in -7 .. 8 (the state is 16-unit-periodic)"""
    return (d + 7) % 16 - 7


class MaskedSum:
    """out = sum_k masks[k] * np.roll(x, steps[k]) + fill: the masks are 0 / 1 and disjoint, fill is 1 on the slots
    no mask covers (the codeword of nibble 0) and None when the masks cover every slot"""

    def __init__(self, steps: List[int], masks: List[np.ndarray]):
        self.steps, self.masks = steps, masks
        rest = 1.0 - np.sum(masks, axis=0)
        self.fill = rest if rest.any() else None

    def apply_slots(self, x: np.ndarray) -> np.ndarray:
        """the sum on a slot vector of nibbles: masked slots take the rolled nibble, filled slots nibble 0"""
        out = np.zeros_like(x)
        for s, m in zip(self.steps, self.masks):
            sel = m > 0.5
            out[sel] = np.roll(x, s)[sel]
        return out

    def apply_values(self, z: np.ndarray) -> np.ndarray:
        """the sum on a slot vector of codewords, as the engine evaluates it"""
        out = sum(m * np.roll(z, s) for s, m in zip(self.steps, self.masks))
        return out if self.fill is None else out + self.fill


class SchedulePlan:
    """the masked rotation sums of one schedule step for a slot layout and byte order (module docstring):
    shift[1], shift[2] (the prefix doubling steps), broadcast (RotWord of word 3 into every word) and wordcopy
    (word 3 into every word, no RotWord: the odd steps of the 256-bit schedule)"""

    def __init__(self, layout, byte_order: Optional[str] = None):
        self.layout = layout
        self.byte_order = byte_order if byte_order is not None else getattr(layout, "byte_order", "plain")
        word_pos(0, 0, self.byte_order)  # validates the order
        self.shift = {k: self._shift_terms(k) for k in (1, 2)}
        self.broadcast = self._broadcast_terms()
        self.wordcopy = self._broadcast_terms(rot=0)

    def _cell(self, pos: int) -> np.ndarray:
        return self.layout.cell_mask(pos % 4, pos // 4).real

    def _sum(self, by_offset: Dict[int, np.ndarray]) -> MaskedSum:
        offs = sorted(by_offset)
        # np.roll(x, s)[j] = x[j - s]: the byte d units above
        return MaskedSum([-d * self.layout.unit for d in offs], [by_offset[d] for d in offs])

    def _shift_terms(self, k: int) -> MaskedSum:
        """word j >= k takes word j - k; the words below k (and the slots that hold no state) take the fill"""
        by: Dict[int, np.ndarray] = {}
        for j in range(k, 4):
            for row in range(4):
                dst = word_pos(row, j, self.byte_order)
                d = _centered(word_pos(row, j - k, self.byte_order) - dst)
                by[d] = by.get(d, np.zeros(self.layout.sc)) + self._cell(dst)
        return self._sum(by)

    def _broadcast_terms(self, rot: int = 1) -> MaskedSum:
        """row rho of every word takes row (rho + rot) % 4 of word 3: rot = 1 is RotWord's broadcast, rot = 0 the
        plain word copy, whose word 3 keeps itself (an identity term, offset 0)"""
        by: Dict[int, np.ndarray] = {}
        for j in range(4):
            for row in range(4):
                dst = word_pos(row, j, self.byte_order)
                d = _centered(word_pos((row + rot) % 4, 3, self.byte_order) - dst)
                by[d] = by.get(d, np.zeros(self.layout.sc)) + self._cell(dst)
        return self._sum(by)

    def sums(self) -> Dict[str, MaskedSum]:
        """the sums of the 128-bit step"""
        return {"shift1": self.shift[1], "shift2": self.shift[2], "broadcast": self.broadcast}

    def sums256(self) -> Dict[str, MaskedSum]:
        """the sums of the 256-bit steps: the 128-bit step's and the word copy"""
        return dict(self.sums(), wordcopy=self.wordcopy)

    def used(self) -> np.ndarray:
        """1 on the slots that hold a state byte"""
        return np.sum([self._cell(p) for p in range(16)], axis=0)

    def rcon_slots(self, r: int) -> Tuple[np.ndarray, np.ndarray]:
        """(hi, lo) nibble slot vectors of round r's constant: RCON[r - 1] on row 0 of word 0 of every state, nibble
        0 elsewhere -- the public operand of AddRoundKey.public"""
        if not 1 <= r <= 10:
            raise ValueError(f"AES-128 schedule rounds are 1..10, got {r}")
        return self.const_slots(r - 1)

    def const_slots(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        """rcon_slots by the constant's index: RCON[i] on row 0 of word 0 of every state (the 256-bit schedule's even
        step r takes i = r // 2 - 1)"""
        if not 0 <= i < len(RCON):
            raise ValueError(f"round constants are RCON[0..{len(RCON) - 1}], got index {i}")
        sel = self._cell(word_pos(0, 0, self.byte_order)) > 0.5
        hi, lo = np.zeros(self.layout.sc, np.uint8), np.zeros(self.layout.sc, np.uint8)
        hi[sel], lo[sel] = int(RCON[i]) >> 4, int(RCON[i]) & 0x0F
        return hi, lo


def schedule_step_slots(x_slots, r: int, layout, byte_order: Optional[str] = None, stages: Optional[dict] = None):
    """round key r from round key r - 1 on nibble slot vectors: x_slots = (hi, lo) uint8 arrays as
    StateEncoder.nibble_slots lays them out; exactly SchedulePlan's rolls, masks and fills, XOR and the S-box in
    clear.  stages (a dict): filled with the (hi, lo) vectors of prefix, sub, rot and out"""
    plan = SchedulePlan(layout, byte_order)
    hi, lo = (np.asarray(v, np.uint8) for v in x_slots)
    rc = plan.rcon_slots(r)
    pre = []
    for v, c in zip((hi, lo), rc):
        x = v ^ c
        y = x ^ plan.shift[1].apply_slots(x)
        pre.append(y ^ plan.shift[2].apply_slots(y))
    s = SBOX[(hi.astype(np.uint8) << 4) | lo]  # on every slot, the ones that hold no state included
    sub = (s >> 4, s & 0x0F)
    rot = tuple(plan.broadcast.apply_slots(v) for v in sub)
    out = tuple(p ^ b for p, b in zip(pre, rot))
    if stages is not None:
        stages.update(prefix=tuple(pre), sub=sub, rot=rot, out=out)
    return out


def schedule_step_bytes(key: np.ndarray, r: int) -> Dict[str, np.ndarray]:
    """the byte model of the debug stages of round r for a (16,) or (B, 16) round key r - 1 in FIPS byte order:
    prefix (word j = w0 ^ ... ^ w_j, rcon_r in row 0), sub (SubBytes of the key), rot (SubWord(RotWord(w3)) in
    every word) and out (round key r)"""
    k = np.asarray(key, np.uint8)
    w = k.reshape(*k.shape[:-1], 4, 4).copy()  # [..., word, row]
    sub = SBOX[k]
    rot = np.repeat(np.roll(SBOX[w[..., 3, :]], -1, axis=-1)[..., None, :], 4, axis=-2)
    w[..., 0, 0] ^= RCON[r - 1]
    pre = np.bitwise_xor.accumulate(w, axis=-2)
    return {"prefix": pre.reshape(k.shape), "sub": sub, "rot": rot.reshape(k.shape), "out": (pre ^ rot).reshape(k.shape)}


def _check_round256(r: int) -> None:
    if not 2 <= r <= 14:
        raise ValueError(f"AES-256 schedule rounds are 2..14, got {r}")


def schedule_step_slots256(prev2, prev1, r: int, layout, byte_order: Optional[str] = None, stages: Optional[dict] = None):
    """round key r = 2..14 of the 256-bit schedule from round keys r - 2 and r - 1 on nibble slot vectors (each a
    (hi, lo) pair as schedule_step_slots takes): the prefix over K_{r-2} -- with RCON[r // 2 - 1] first when r is even,
    K_{r-2} itself when r is odd -- XOR SubBytes(K_{r-1}) moved by the broadcast (r even) or the word copy (r odd).
    stages as schedule_step_slots'"""
    _check_round256(r)
    plan = SchedulePlan(layout, byte_order)
    hi2, lo2 = (np.asarray(v, np.uint8) for v in prev2)
    hi1, lo1 = (np.asarray(v, np.uint8) for v in prev1)
    rc = plan.const_slots(r // 2 - 1) if r % 2 == 0 else None
    pre = []
    for i, v in enumerate((hi2, lo2)):
        x = v if rc is None else v ^ rc[i]
        y = x ^ plan.shift[1].apply_slots(x)
        pre.append(y ^ plan.shift[2].apply_slots(y))
    s = SBOX[(hi1.astype(np.uint8) << 4) | lo1]
    sub = (s >> 4, s & 0x0F)
    move = plan.broadcast if r % 2 == 0 else plan.wordcopy
    rot = tuple(move.apply_slots(v) for v in sub)
    out = tuple(p ^ b for p, b in zip(pre, rot))
    if stages is not None:
        stages.update(prefix=tuple(pre), sub=sub, rot=rot, out=out)
    return out


def schedule_step_bytes256(prev2: np.ndarray, prev1: np.ndarray, r: int) -> Dict[str, np.ndarray]:
    """the byte model of the debug stages of round r = 2..14 of the 256-bit schedule for (16,) or (B, 16) round keys
    r - 2 and r - 1 in FIPS byte order: prefix (over K_{r-2}, RCON[r // 2 - 1] in row 0 when r is even), sub (SubBytes
    of K_{r-1}), rot (SubWord(RotWord(w3)) of K_{r-1} in every word when r is even, SubWord(w3) when r is odd) and
    out (round key r)"""
    _check_round256(r)
    k2, k1 = np.asarray(prev2, np.uint8), np.asarray(prev1, np.uint8)
    w = k2.reshape(*k2.shape[:-1], 4, 4).copy()  # [..., word, row]
    sub = SBOX[k1]
    last = sub.reshape(*k1.shape[:-1], 4, 4)[..., 3, :]
    rot = np.repeat((np.roll(last, -1, axis=-1) if r % 2 == 0 else last)[..., None, :], 4, axis=-2)
    if r % 2 == 0:
        w[..., 0, 0] ^= RCON[r // 2 - 1]
    pre = np.bitwise_xor.accumulate(w, axis=-2)
    return {"prefix": pre.reshape(k2.shape), "sub": sub, "rot": rot.reshape(k1.shape), "out": (pre ^ rot).reshape(k2.shape)}


class EncryptedRoundKeys:
    """11, 13 or 15 layout-tagged (hi, lo) pairs, the AES-128 / 192 / 256 round keys under FHE (the pipeline runs
    len - 1 rounds), with the caches a pipeline keeps per key schedule: `packed` (one entry per round key; the middle
    rounds 1..len - 2 in the packed form, filled on first use) and `key_basis` (round -> the packed key's dropped form
    and XOR4 basis, AESPipeline._ark_packed).  Every AESPipeline method that takes round keys takes one of these; the
    server then never holds a key byte in clear."""

    COUNTS = (11, 13, 15)

    def __init__(self, pairs, layout):
        pairs = [tuple(p) for p in pairs]
        if len(pairs) not in self.COUNTS or any(len(p) != 2 for p in pairs):
            raise ValueError("AES takes 11 round keys (AES-128), 13 (AES-192) or 15 (AES-256), each a (hi, lo) "
                             f"ciphertext pair; got {len(pairs)}")
        for p in pairs:
            check_layout(layout, *p)
            tag_layout(layout, *p)
        self.pairs, self.layout = pairs, layout
        self.raw = None  # no key byte in clear (ClearRoundKeys has them)
        self.packed: List[Any] = [None] * len(pairs)
        self.key_basis: Dict[int, Dict[str, Any]] = {}

    @classmethod
    def from_pairs(cls, pairs, layout) -> "EncryptedRoundKeys":
        """round keys the client expanded and encrypted itself (StateEncoder.encode of each, in `layout`)"""
        return cls(pairs, layout)

    def dump_seeded(self, ctx):
        """the 22 (26, 30) ciphertexts as dump_ct_seeded records, in (round, hi / lo) order: every
        pair must be a seeded fresh encryption (StateEncoder.encode_many(..., seeded=True)); half of the dump_ct bytes"""
        from state_encoder import dump_ct_seeded
        return [dump_ct_seeded(ctx, c) for pr in self.pairs for c in pr]

    @classmethod
    def load_seeded(cls, ctx, records, layout) -> "EncryptedRoundKeys":
        """the inverse of dump_seeded on the receiving context: records with consecutive seed ids (one
        encrypt_seeded_many call made them) go through one batched import"""
        from state_encoder import load_cts_seeded
        records = list(records)
        if len(records) not in tuple(2 * n for n in cls.COUNTS):
            raise ValueError("AES takes 11, 13 or 15 round keys: 22 seeded records (26, 30), (hi, lo) per round; "
                             f"got {len(records)}")
        cts = load_cts_seeded(ctx, records)
        return cls([(cts[2 * r], cts[2 * r + 1]) for r in range(len(records) // 2)], layout)

    def __len__(self) -> int:
        return len(self.pairs)

    def __getitem__(self, r: int):
        return self.pairs[r]


class ClearRoundKeys:
    """the key schedule an AESPipeline keeps for CLEAR round keys, in EncryptedRoundKeys' shape: `pairs` (the keys
    encrypted by the pipeline, as the reference does), `packed` and `key_basis` as there, and what only clear keys can
    have: `raw` (the uint8 key arrays) and `fused` ((round, direction) -> the encrypted pair of the key permuted by
    (Inv)ShiftRows, AESPipeline._fused_key).  A pipeline keeps the most recent one and reuses it while `matches`."""

    def __init__(self, raw, pairs):
        self.raw, self.pairs = raw, pairs
        self.tag = self.tag_of(raw)
        self.packed: List[Any] = [None] * len(pairs)
        self.key_basis: Dict[int, Dict[str, Any]] = {}
        self.fused: Dict[Tuple[int, int], Tuple[Any, Any]] = {}

    @staticmethod
    def tag_of(raw) -> bytes:
        """the round-key count, then the bytes of all keys: schedules of different lengths never match"""
        return bytes([len(raw)]) + b"".join(k.tobytes() for k in raw)

    def matches(self, raw) -> bool:
        return self.tag == self.tag_of(raw)


class KeyExpansion:
    """the schedule on an AESPipeline's own modules (xor4 through ark / ark.public, sub, _renorm_pair, _floor,
    encoder.layout), so it follows use_hard_renorm_between_steps, true_fhe, states and fips.  Per round of the
    128-bit schedule: 4 XOR4 pairs (one of them public), one SubBytes, 6 masked rotation sums, 5 renorms.  The
    256-bit schedule (step256, expand256) runs the same pieces from two round keys: its even steps
    cost what a 128-bit step costs, its odd steps one XOR4 pair (the public one) and one renorm less."""

    def __init__(self, pipe):
        if pipe.pairs > 1:
            raise ValueError("KeyExpansion: multi-pair batches (pairs > 1) take no public operands")
        ctx = pipe.ctx
        if getattr(ctx, "rot_pt_affine", None) is None:
            raise TypeError("KeyExpansion needs a context with rot_pt_affine (engine_context.EngineContext)")
        self.pipe, self.ctx = pipe, ctx
        self.layout = pipe.encoder.layout
        self.plan = SchedulePlan(self.layout)
        self._pts: Dict[str, Any] = {}
        for name in self.plan.sums():
            self._plaintexts(name)

    def _plaintexts(self, name: str):
        """(mask plaintexts, fill plaintext or None) of a sum of the plan, encoded once (the word copy's on the first
        256-bit step)"""
        if name not in self._pts:
            s = self.plan.sums256()[name]
            self._pts[name] = ([self.ctx.encode(m) for m in s.masks], None if s.fill is None else self.ctx.encode(s.fill))
        return self._pts[name]

    def _move(self, name: str, ct_hi, ct_lo):
        """one masked rotation sum of the plan on both halves (one level)"""
        steps = self.plan.sums256()[name].steps
        masks, fill = self._plaintexts(name)
        return tuple(self.ctx.rot_pt_affine(c, steps, [masks], [fill])[0] for c in (ct_hi, ct_lo))

    def _prefix(self, x):
        """the prefix XOR over the words of x (a clean pair at NEED_SR_ARK) in two doubling steps, at NEED_XOR"""
        p = self.pipe
        fl = p._floor()
        y = p._renorm_pair(*p.ark(*x, *self._move("shift1", *x), out_level=fl), level=NEED_SR_ARK)
        return p._renorm_pair(*p.ark(*y, *self._move("shift2", *y), out_level=fl), level=NEED_XOR)

    def _finish(self, pre, key, move: str, r: int, debug):
        """round key r = pre ^ move(SubBytes(key)), with the stages logged"""
        p = self.pipe
        p._log_pair(debug, f"ks.r{r}.prefix", *pre)
        sub = p._sub_renorm(key, level=NEED_SR_ARK)
        p._log_pair(debug, f"ks.r{r}.sub", *sub)
        rot = self._move(move, *sub)
        p._log_pair(debug, f"ks.r{r}.rot", *rot)
        out = tag_layout(self.layout, *p._renorm_pair(*p.ark(*pre, *rot, out_level=p._floor())))
        p._log_pair(debug, f"ks.r{r}.out", *out)
        return out

    def step(self, key, r: int, debug=None):
        """round key r (a clean pair at the level the last renorm hands out) from round key r - 1"""
        p = self.pipe
        x = p.ark.public(*key, *self.plan.rcon_slots(r), out_level=p._floor())
        x = p._renorm_pair(*x, level=NEED_SR_ARK)  # a masked rotation sum, then an XOR4
        return self._finish(self._prefix(x), key, "broadcast", r, debug)

    def step256(self, prev2, prev1, r: int, debug=None):
        """round key r = 2..14 of the 256-bit schedule from round keys r - 2 and r - 1 (clean pairs):
        r even: prefix(K_{r-2} ^ RCON[r // 2 - 1]) ^ broadcast(SubBytes(K_{r-1})), a 128-bit step on two keys;
        r odd: prefix(K_{r-2}) ^ wordcopy(SubBytes(K_{r-1})) -- no constant, so no public XOR and no renorm after
        it: the prefix starts from K_{r-2} itself, dropped to the level that renorm would have handed out"""
        _check_round256(r)
        p = self.pipe
        if r % 2 == 0:
            x = p.ark.public(*prev2, *self.plan.const_slots(r // 2 - 1), out_level=p._floor())
            x = p._renorm_pair(*x, level=NEED_SR_ARK)
            return self._finish(self._prefix(x), prev1, "broadcast", r, debug)
        x = tag_layout(self.layout, *(drop_to(self.ctx, c, NEED_SR_ARK) for c in prev2))
        return self._finish(self._prefix(x), prev1, "wordcopy", r, debug)

    def expand(self, key_hi, key_lo, debug: Optional[Dict[str, Any]] = None) -> EncryptedRoundKeys:
        """the 11 round keys of the encrypted key (hi, lo) (AESPipeline.encrypt_key; with states > 1 every state
        holds its own key and gets its own schedule).  Round key 0 is the input, renormalised; every key sits at
        the level the pipeline's renorm hands out with no target (the fresh level in the secret-key renorm mode)."""
        check_layout(self.layout, key_hi, key_lo)
        if debug is not None:
            debug.clear()
        keys = [tag_layout(self.layout, *self.pipe._renorm_pair(key_hi, key_lo))]
        for r in range(1, 11):
            keys.append(self.step(keys[-1], r, debug))
        return EncryptedRoundKeys(keys, self.layout)

    def expand256(self, key_hi, key_lo, key_hi1, key_lo1, debug: Optional[Dict[str, Any]] = None) -> EncryptedRoundKeys:
        """the 15 round keys of an encrypted 32-byte key: (key_hi, key_lo) holds bytes 0..15, (key_hi1, key_lo1) bytes
        16..31 (AESPipeline.encrypt_key).  Round keys 0 and 1 are the inputs, renormalised; keys 2..14 come from
        step256, every one at the level expand's keys sit at.  Debug stages ks.r{r}.{prefix,sub,rot,out}, r = 2..14"""
        check_layout(self.layout, key_hi, key_lo, key_hi1, key_lo1)
        if debug is not None:
            debug.clear()
        keys = [tag_layout(self.layout, *self.pipe._renorm_pair(h, l)) for h, l in ((key_hi, key_lo), (key_hi1, key_lo1))]
        for r in range(2, 15):
            keys.append(self.step256(keys[-2], keys[-1], r, debug))
        return EncryptedRoundKeys(keys, self.layout)
