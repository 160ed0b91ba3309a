"""AESPipeline: AES round orchestration on CKKS/Zeta16 (REF/pipeline.py:17-254).

The key size follows the round keys: 11 / 13 / 15 of them (AES-128 / 192 / 256), clear or encrypted, run 10 / 12 / 14
rounds in every method that takes round keys; any other count is a ValueError.  The reference runs AES-128 only.

Drop-in for the reference class: same constructor, same coefficient keys ('xor4',
'sub_hi', 'sub_lo', 'inv_sub_hi', 'inv_sub_lo'), same step order, optional renorm
between steps, per-stage debug snapshots.

Documented deviation: the shipped decrypt (REF/pipeline.py:230-237)
never applies InvMixColumns, so it cannot invert encrypt.  ``decrypt`` here inserts it
after AddRoundKey as the reference README prescribes (REF/README.md:87-94);
``with_inv_mix_columns=False`` reproduces the shipped order.

``fuse_sub_ark=True`` evaluates SubBytes ⊕ AddRoundKey as one fused LUT per nibble
(sub_bytes_ark.py, SURVEY.md §8(f)4, REF/README.md:133-135): the last encrypt round and every
decrypt round, across the (Inv)ShiftRows between them via permuted round keys; one XOR4 pair
and one renorm fewer per fused step, the same bytes.

``fuse_sr_mc=True`` merges ShiftRows into MixColumns' rotations (shiftrows_mixcolumns.py, the
GHS12 refinement of REF/README.md:137-138): three hoisted rotations per nibble instead of six.

``true_fhe=True`` replaces every secret-key renorm by a bootstrap + homomorphic Zeta16 snap
(zeta16_noise_reducer.BootstrapSnap): the XOR4 coefficients are normalised
by 1/256 (REF/gen/generate_xor4_coeffs.py:17) so every LUT output has unit magnitude,
MixColumns' / InvMixColumns' final bootstraps merge into their last renorm, and decrypt
applies each InvShiftRows before the renorm that precedes InvSubBytes (the snap leaves
exactly SubBytes' 13 levels).  No secret key is used between encryption and decryption.

``packed_xor`` (default: wherever it applies) runs MixColumns' XOR stage and the AddRoundKey
after it on packed states -- hi and lo side by side in ONE ciphertext, the XOR4 LUT being the
same for both halves (MixColFinal.mix_packed): single XOR4s instead of pairs,
single-ciphertext renorms, one sparse bootstrap; the renorm after AddRoundKey unpacks into the
(hi, lo) pair SubBytes reads (``packed_xor=False`` runs the reference's pair steps).  On either path a
debug dict logs the stages of the very run an unlogged call makes: same levels, folds and hand-overs.

``states`` = B > 1 runs B independent AES states per ciphertext pair in the slot-packed
layout (state_encoder.py): ``encrypt`` / ``decrypt`` take and return
(B, 16) arrays through the same step sequence, and a (16,) round key is shared by all B
states (a (B, 16) key array gives each state its own).

``fips=True`` computes FIPS-197 AES (128, 192 or 256 by the key count) instead of the reference's cipher (whose MixColumns mixes along
rows).  With T the 4 x 4 byte transpose, fips_encrypt(p, rks) = T(E'(T p, [T rk_r])) where
E' is this pipeline's round sequence with ShiftColumns = T . ShiftRows . T in place of ShiftRows
(shift_columns.py) and MixColumns unchanged; decrypt likewise with the inverses.  So the mode is the two
ShiftColumns modules plus a byte transpose wherever clear bytes enter or leave (the encoder's
byte_order="transposed": states, round keys, counter blocks, public AES ciphertext bytes, decode and the debug
snapshots).  Its pairs are tagged transposed and refused by a plain pipeline (check_layout).  ``fuse_sub_ark``,
``fuse_sr_mc`` and ``pairs`` > 1 are not available with it (ValueError).

Real-valued slots (xor_value_lut.py): ``transcipher_values`` / ``to_values`` return ONE ciphertext whose
state slots hold gain * byte as real numbers (read back by ``encoder.decode_values``) instead of the Zeta16 pair -- the
last public XOR of counter mode fused with the value decode, no renorm after the keystream.  ``dtype`` / ``gain`` /
``offset`` read the bytes as int8 / uint8 or 16-bit words of either sign and byte order, with per-word
gains and offsets, for no further level.  ``transcipher_linear`` / ``to_linear`` apply a 16 x 16 matrix
per state to the decoded bytes inside the same step: the matrix's cyclic diagonals as weight groups of the decode.
``transcipher_lut`` / ``to_lut`` put an arbitrary 256-entry table of the byte in the slots instead, for
one ct x ct level more; ``transcipher_lut_bank`` / ``to_lut_bank`` take a bank of such tables, a table
per byte, and return several outputs of one keystream.

Encrypted round keys (key_expansion.py): every method that takes ``round_keys`` takes either the list of
11 (13, 15) clear byte arrays (encrypted here, as the reference does) or a ``key_expansion.EncryptedRoundKeys`` -- as many
ciphertext pairs the server never saw in clear: ``expand_key(*encrypt_key(master))`` derives them homomorphically from ONE
encrypted 16-byte key, or from the two halves of an encrypted 32-byte key;
``EncryptedRoundKeys.from_pairs`` wraps keys the client expanded itself (the route of AES-192).  Their packed forms are
built homomorphically and cached on the object.  Refused (ValueError): keys of another layout or byte order,
``pairs`` > 1, ``fuse_sub_ark`` (its fused keys permute clear key bytes).
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional

import numpy as np

from add_round_key import AddRoundKey
from invmixcolumns_fhe import InvMixColumnsFHE
from key_expansion import ClearRoundKeys, EncryptedRoundKeys, KeyExpansion
from inv_shiftrows import InvShiftRows
from mixcol_final import MixColFinal
from shift_rows import ShiftRows
from state_encoder import LUT_VALUE_TAG, StateEncoder, check_layout, tag_layout, tag_value_dtype
from shift_rows import shift_rows_bytes
from shiftrows_mixcolumns import ShiftRowsMixColumnsFusedEnc
from sub_bytes_ark import SubBytesARK
from sub_bytes_lut import SubBytesLUT
from utils import (pair, FOLDS, SHIFTROWS_DEPTH, NEED_GF, NEED_ISR_ISB, NEED_SR_ARK, NEED_SR_MIX, NEED_SUB_ARK_SR, NEED_SUBBYTES, NEED_XOR,
                   RENORM_FLOOR)
from xor4_lut import XOR4LUT

# AESFHE_KEY_BASIS=0: the packed round keys' XOR4 bases rebuilt in every AddRoundKey (A/B runs)
_KEY_BASIS = os.environ.get("AESFHE_KEY_BASIS", "1") != "0"
# AESFHE_FHE_SB_NIB=0: true-FHE mode keeps the reference's 8 -> 4 (Inv)SubBytes (depth 13, double snaps)
# instead of the nibble-bivariate form (A/B runs)
_FHE_NIB = os.environ.get("AESFHE_FHE_SB_NIB", "1") != "0"


def round_count(round_keys) -> int:
    """Nr = 10 / 12 / 14 for 11 / 13 / 15 round keys (AES-128 / 192 / 256), clear or EncryptedRoundKeys; any other
    count is a ValueError, raised before any GPU work"""
    n = len(round_keys)
    if n not in EncryptedRoundKeys.COUNTS:
        raise ValueError(f"AES takes 11 round keys (AES-128), 13 (AES-192) or 15 (AES-256), got {n}")
    return n - 1


# The shared bodies of AESPipeline's transcipher_* and to_* methods.  Module functions, so that they serve any object
# with the pipeline's attributes (the CPU tests bind single methods to stand-ins).  `build` makes the LUT object and
# raises the ValueErrors of its own arguments; every refusal comes before any GPU work, in the order written here.
def _transcipher_with(pipe, name: str, aes_ct, nonce12, counter0: int, round_keys, build):
    pipe._no_pairs(name)
    round_count(round_keys)  # 11 / 13 / 15 keys
    nib = pipe.encoder.nibble_slots(aes_ct)  # checks the shape
    lut = build()
    ks = pipe.ctr_keystream(nonce12, counter0, round_keys)
    return lut.apply_public(*ks, *nib)


def _convert_with(pipe, name: str, ct_hi, ct_lo, build):
    pipe._no_pairs(name)
    check_layout(pipe.layout, ct_hi, ct_lo)
    return build().apply(ct_hi, ct_lo)


def _values_lut(pipe, dtype, gain, offset):
    """the LUT of transcipher_values / to_values: the typed one, or XorValueLUT for plain unsigned bytes"""
    typed = pipe._typed_lut(dtype, gain, offset)
    return typed if typed is not None else pipe._value_lut(1.0 / 256.0 if gain is None else gain)


class AESPipeline:
    def __init__(self, ctx, coeffs: Dict[str, Any], *, mixcolumns: MixColFinal | None = None,
                 inv_mixcolumns: InvMixColumnsFHE | None = None, use_hard_renorm_between_steps: bool = False,
                 with_inv_mix_columns: bool = True, states: int = 1, fuse_sub_ark: bool = False,
                 fuse_sr_mc: bool = False, true_fhe: bool = False, periodic: bool | None = None,
                 packed_xor: bool | None = None, pairs: int = 1, fips: bool = False):
        self.ctx = ctx
        self.fips = bool(fips)
        if fips and (fuse_sub_ark or fuse_sr_mc or pairs > 1):
            raise ValueError("fips=True does not combine with fuse_sub_ark, fuse_sr_mc or pairs > 1")
        # an evaluation-only context (EngineContext.from_evaluation_keys) holds no secret: the secret-key renorm is
        # refused here, not deep inside the first round; true_fhe=True (bootstrap + snap) is its renorm
        if getattr(ctx, "evaluation_only", False) and use_hard_renorm_between_steps:
            raise ValueError("use_hard_renorm_between_steps=True needs the secret key: an evaluation-only context "
                             "renormalises with true_fhe=True (bootstrap + snap) only")
        self.states = states
        # pairs > 1: a multi-pair batch -- `pairs` ciphertext pairs of `states` states each, run as
        # ONE stacked pair through every step (state_encoder.StateEncoder)
        self.pairs = pairs
        # periodic layout (state_encoder.SlotLayout): default on where the engine
        # has the sparse-slot bootstrap and the state count is a power of two
        if periodic is None:
            periodic = getattr(ctx, "bootstrap_pair_sparse", None) is not None and states & (states - 1) == 0
            for mod in (mixcolumns, inv_mixcolumns):
                lay = getattr(mod, "layout", None)
                if lay is not None:
                    periodic = lay.periodic
        self.encoder = (StateEncoder(ctx, states, periodic=periodic, pairs=pairs, byte_order="transposed") if fips else
                        StateEncoder(ctx, states, periodic=periodic, pairs=pairs))
        self.layout = self.encoder.layout
        self.sc = ctx.engine.slot_count
        self.stride = self.layout.unit
        self.true_fhe = true_fhe
        # true-FHE: unit-magnitude XOR4 (REF/gen/generate_xor4_coeffs.py:17), so the snap sees codewords
        self.xor4 = XOR4LUT(ctx, np.asarray(coeffs["xor4"]) / 256.0 if true_fhe else coeffs["xor4"])
        self.sub = SubBytesLUT(ctx, coeffs["sub_hi"], coeffs["sub_lo"])
        self.isub = SubBytesLUT(ctx, coeffs["inv_sub_hi"], coeffs["inv_sub_lo"]) if "inv_sub_hi" in coeffs else None
        if fips:
            from shift_columns import InvShiftColumns, ShiftColumns
            self.shift = ShiftColumns(ctx, states=states, layout=self.layout)
            self.invshift = InvShiftColumns(ctx, states=states, layout=self.layout)
        else:
            self.shift = ShiftRows(ctx, states=states, layout=self.layout)
            self.invshift = InvShiftRows(ctx, states=states, layout=self.layout)
        self.mix = mixcolumns if mixcolumns is not None else MixColFinal(ctx, self.xor4, states=states, layout=self.layout)
        self.invmix = (inv_mixcolumns if inv_mixcolumns is not None else
                       InvMixColumnsFHE(ctx, self.xor4, states=states, layout=self.layout))
        for mod in (self.mix, self.invmix):
            enc = getattr(mod, "enc", None)
            if enc is not None and getattr(enc, "states", 1) != states:
                raise ValueError("mixcolumns / inv_mixcolumns were built for a different states-per-ciphertext count")
            lay = getattr(mod, "layout", None)
            if lay is not None and not self.layout.same(lay):
                raise ValueError("mixcolumns / inv_mixcolumns were built for a different slot layout")
        self.ark = AddRoundKey(self.xor4)
        self.snapper = None
        self.use_hard_renorm_between_steps = use_hard_renorm_between_steps
        self.with_inv_mix_columns = with_inv_mix_columns
        # the key schedule of the last call (_prepare_round_keys): a ClearRoundKeys or the caller's EncryptedRoundKeys
        self._schedule: ClearRoundKeys | EncryptedRoundKeys | None = None
        self._fold_perms: Dict[Any, Any] = {}  # shift module -> its slot_perm() (_fold_perm)
        self.fuse_sub_ark = fuse_sub_ark
        if fuse_sub_ark:
            self.sbark = SubBytesARK(self.sub, coeffs["xor4"])
            self.isbark = SubBytesARK(self.isub, coeffs["xor4"]) if self.isub is not None else None
        self.srmc = None
        if fuse_sr_mc:
            if not hasattr(self.mix, "mix_rotated"):
                raise TypeError("fuse_sr_mc needs a MixColFinal (mix_rotated) as mixcolumns")
            self.srmc = ShiftRowsMixColumnsFusedEnc(ctx, self.mix, states)
        # packed XOR stage of encrypt's middle rounds 1..nr - 1; AESFHE_PACKED_XOR=0 for A/B
        if packed_xor is None:
            packed_xor = os.environ.get("AESFHE_PACKED_XOR", "1") != "0"
        self.packed_xor = bool(packed_xor and use_hard_renorm_between_steps and not true_fhe and self.srmc is None
                               and hasattr(self.mix, "packed_ok") and self.mix.packed_ok())
        # the same for decrypt's middle rounds nr - 1..1: AddRoundKey + InvMixColumns (with_inv_mix_columns)
        self.packed_dec = bool(self.packed_xor and with_inv_mix_columns and not fuse_sub_ark
                               and hasattr(self.invmix, "packed_ok") and self.invmix.packed_ok())
        # the level encrypt's renorms hand SubBytes: one above its depth in renorm mode, so that it
        # takes the bivariate giant-step form (sub_bytes_lut._outputs_biv; AESFHE_SB_BIV=0 for A/B)
        self.need_sub = NEED_SUBBYTES
        fresh = getattr(ctx.engine, "fresh_level", None)
        # (Inv)SubBytes in the nibble-bivariate form (sub_bytes_lut: depth LUT2_DEPTH instead of 13) in the
        # secret-key renorm mode: its inputs come from a renorm, so they are handed out 9 levels lower
        for lut in (self.sub, self.isub):
            if lut is not None and not fuse_sub_ark:
                lut.use_nibble = bool(use_hard_renorm_between_steps and not true_fhe or true_fhe and _FHE_NIB)
        if true_fhe:
            from zeta16_noise_reducer import BootstrapSnap
            # one snap per renorm with the nibble-bivariate (Inv)SubBytes, two where the reference's
            # 8 -> 4 form's ~3e-2 output errors need them (zeta16_noise_reducer.BootstrapSnap)
            self.snapper = BootstrapSnap(ctx, period=self.layout.boot_period, max_snaps=1 if self.sub.nibble_on() else 2)
            quad = self.snapper.apply_quad if self.snapper.quad_ok() else None
            for enc in (self.encoder, getattr(self.mix, "enc", None), getattr(self.invmix, "enc", None)):
                if enc is not None:
                    enc.renorm_hook = self.snapper.apply_pair
                    enc.renorm_quad_hook = quad
        if self.sub.nibble_on():
            self.need_sub = RENORM_FLOOR + self.sub.need_depth()
        elif (use_hard_renorm_between_steps and not true_fhe and fresh is not None and getattr(ctx, "fused_luts", False)
                and os.environ.get("AESFHE_SB_BIV", "1") != "0"):
            self.need_sub = min(NEED_SUBBYTES + 1, fresh)
        # InvShiftRows -> InvSubBytes (decrypt): the inverse LUT's depth + the masked rotations
        self.need_isr_isb = (RENORM_FLOOR + self.isub.need_depth() + SHIFTROWS_DEPTH
                             if self.isub is not None and self.isub.nibble_on() else NEED_ISR_ISB)

    # ---------------------------------------------------------------- utils
    def _renorm_pair(self, hi, lo, level=None):
        """renorm between steps; `level` = what the next step needs (utils.NEED_*; None = fresh)"""
        if self.true_fhe or self.use_hard_renorm_between_steps:
            return self.encoder.renorm(hi, lo, level)
        return hi, lo

    def _floor(self) -> Optional[int]:
        """output level a step needs when a renorm follows it (utils.RENORM_FLOOR), else None"""
        if self.true_fhe:
            return 1  # the bootstrap reads any level; decrypt's InvShiftRows needs one above 0
        return RENORM_FLOOR if self.use_hard_renorm_between_steps else None

    def _ark_renorm(self, ct, key_pair, level=None):
        """AddRoundKey then renorm: the XOR4s run on inputs dropped just above the floor"""
        return self._renorm_pair(*self.ark(*ct, *key_pair, out_level=self._floor()), level=level)

    def _sub_level(self, level):
        """the level the renorm after (Inv)SubBytes hands out, `level` but in true-FHE mode: SubBytes' ~3e-2 output
        errors get two snaps (ShiftRows + the GF multipliers need 6 levels, MixColumns renormalises after them)"""
        return NEED_SR_ARK if self.true_fhe else level

    def _sub_renorm(self, ct, inverse: bool = False, level=None):
        lut = self.isub if inverse else self.sub
        if lut is None:
            raise KeyError("inv_sub_hi")
        return self._renorm_pair(*self._sub_apply(ct, defer_conj=True, lut=lut), level=self._sub_level(level))

    def _encode_key(self, key_bytes: np.ndarray, seeded: bool = False):
        key_bytes = np.asarray(key_bytes, dtype=np.uint8)
        if self.states > 1 and key_bytes.shape == (16,):
            key_bytes = np.broadcast_to(key_bytes, (self.states, 16))
        assert key_bytes.shape == ((16,) if self.states == 1 else (self.states, 16))
        return self.encoder.encode(key_bytes, seeded=True) if seeded else self.encoder.encode(key_bytes)

    def encrypt_key(self, master: np.ndarray, seeded: bool = False):
        """client side: the (hi, lo) encryption of a (16,) AES-128 key, or of a (states, 16) array with one key
        per state (a (16,) key is shared by all states, as _encode_key broadcasts it) -- expand_key's input.
        A (32,) or (states, 32) AES-256 key gives the 4-tuple (hi0, lo0, hi1, lo1): the pairs of key bytes 0..15 and
        16..31, what expand_key takes as its four ciphertexts.  A 24-byte key is a ValueError: the AES-192 schedule is
        not expanded homomorphically (EncryptedRoundKeys.from_pairs takes its 13 client-expanded keys).
        seeded=True: one batched seeded symmetric encryption (of all four ciphertexts for a 32-byte
        key), the ciphertexts then cross the wire as halves (state_encoder.dump_ct_seeded / load_ct_seeded)"""
        if seeded and self.pairs > 1:
            raise ValueError("encrypt_key: seeded encryption of multi-pair batches (pairs > 1) is not supported")
        n = np.shape(master)[-1] if np.ndim(master) else 0
        if n == 24:
            raise ValueError("encrypt_key: a 24-byte AES-192 key is not expanded homomorphically; expand it on the "
                             "client and wrap its 13 encrypted round keys with EncryptedRoundKeys.from_pairs")
        if n != 32:
            return self._encode_key(master, seeded)
        key = np.asarray(master, dtype=np.uint8)
        if self.states > 1 and key.shape == (32,):
            key = np.broadcast_to(key, (self.states, 32))
        if key.shape != ((32,) if self.states == 1 else (self.states, 32)):
            raise ValueError(f"encrypt_key: a (32,) AES-256 key or one per state, ({self.states}, 32); got {key.shape}")
        halves = [key[..., :16], key[..., 16:]]
        if seeded:
            (hi0, lo0), (hi1, lo1) = self.encoder.encode_many(halves, seeded=True)
        else:
            (hi0, lo0), (hi1, lo1) = (self.encoder.encode(h) for h in halves)
        return hi0, lo0, hi1, lo1

    def expand_key(self, key_hi, key_lo, key_hi1=None, key_lo1=None, debug: Dict[str, Any] | None = None) -> EncryptedRoundKeys:
        """the 11 round keys of an encrypted AES-128 key, derived homomorphically (key_expansion.KeyExpansion,
        DESIGN.md §3.19): what encrypt / decrypt / encrypt_public / ctr_keystream / transcipher take as
        round_keys in place of clear bytes.  With the second pair (key_hi1, key_lo1) -- expand_key(*encrypt_key(key32))
        -- the 15 round keys of an encrypted AES-256 key: keys 0 and 1 are the inputs, renormalised.
        A debug dict gets the stages ks.r{r}.{prefix,sub,rot,out} (r = 1..10, or 2..14 for AES-256)."""
        if (key_hi1 is None) != (key_lo1 is None):
            raise ValueError("expand_key: the second half of an AES-256 key is a (hi, lo) pair, both or neither")
        if getattr(self, "_key_expansion", None) is None:
            self._key_expansion = KeyExpansion(self)
        if key_hi1 is None:
            return self._key_expansion.expand(key_hi, key_lo, debug)
        return self._key_expansion.expand256(key_hi, key_lo, key_hi1, key_lo1, debug)

    def _check_encrypted_keys(self, erk: EncryptedRoundKeys) -> None:
        if self.pairs > 1:
            raise ValueError("encrypted round keys: multi-pair batches (pairs > 1) are not supported")
        if self.fuse_sub_ark:
            raise ValueError("encrypted round keys do not combine with fuse_sub_ark (its fused keys permute clear key bytes)")
        for pr in erk.pairs:  # tagged with erk.layout: another slot layout or byte order is refused here
            check_layout(self.layout, *pr)
        if not self.layout.same(erk.layout):  # ciphertexts that carry no tag (the CPU oracle's)
            raise ValueError("encrypted round keys were made for another slot layout or byte order")

    def _prepare_round_keys(self, round_keys):
        """the encrypted (hi, lo) pair of every round key: 11, 13 or 15 of them, and the callers run len - 1 rounds.
        Everything cached per key schedule (the pairs, the packed keys, their XOR4 bases, the fused keys) lives on ONE
        object, self._schedule: the caller's EncryptedRoundKeys, kept by identity with nothing encoded, or the most
        recent ClearRoundKeys, reused while the key count and the bytes of all keys match"""
        round_count(round_keys)
        if isinstance(round_keys, EncryptedRoundKeys):
            self._check_encrypted_keys(round_keys)
            self._schedule = round_keys
            return round_keys.pairs
        raw = [np.array(k, dtype=np.uint8) for k in round_keys]
        if not (isinstance(self._schedule, ClearRoundKeys) and self._schedule.matches(raw)):
            self._schedule = ClearRoundKeys(raw, [self._encode_key(k) for k in raw])
        return self._schedule.pairs

    def _ark_packed(self, x, r: int, defer_conj: bool = False):
        """AddRoundKey on a packed state: XOR4(x, packed round key r).  The key's level drop and
        std basis (its conjugate and power chain) are built once per key schedule and round and
        reused by every later encrypt / decrypt with the same keys (AESFHE_KEY_BASIS=0: rebuilt
        per call) -- the XOR4 then forms only the state's powers.  defer_conj: the result goes into
        renorm_unpack, which takes the split LUT's S1 + conj(S2) unsummed (utils.ConjSum)"""
        key = self._packed_round_key(r)
        if not _KEY_BASIS:
            return self.xor4.apply(x, key, out_level=self._floor())
        kb = self._schedule.key_basis.setdefault(r, {})
        return self.xor4.apply(x, key, out_level=self._floor(), keep_b=kb, defer_conj=bool(defer_conj and FOLDS.conj))

    def _fold_perm(self, shift, ct):
        """the byte permutation of `shift` (self.shift or self.invshift) when the renorm before it can fold it
        (utils.FOLDS.sr: off in the strict default; secret-key renorm mode, one period-16 state pair on the device),
        else None.  A debug run keeps the fold and logs what it can (no separate log of the renorm's own output)"""
        if not FOLDS.sr or self.true_fhe or not self.use_hard_renorm_between_steps:
            return None
        if shift not in self._fold_perms:
            sp = getattr(shift, "slot_perm", None)
            self._fold_perms[shift] = sp() if sp is not None else None
        perm = self._fold_perms[shift]
        ok = getattr(self.encoder, "renorm_perm_ok", None)
        if perm is None or ok is None:
            return None
        return perm if ok(ct[0].s1 if hasattr(ct[0], "s1") else ct[0]) else None

    def _sr_entry_ok(self) -> bool:
        """ShiftRows runs inside MixColumns' packed entry (MixColFinal.sr_entry): the rot form with its
        GF pair low, this pipeline's own ShiftRows layout (AESFHE_SR_MC_ENTRY=0: a separate step)"""
        from mixcol_final import SR_MC_ENTRY
        return (SR_MC_ENTRY and hasattr(self.mix, "sr_entry") and os.environ.get("AESFHE_MC_FORM", "rot") == "rot"
                and self.layout.packable and getattr(self.shift, "direction", None) == -1)

    def _sub_apply(self, ct, defer_conj: bool = False, lut=None):
        """(Inv)SubBytes (lut, default self.sub) on the pair down to the renorm floor; defer_conj (the
        output goes straight into _renorm_pair): the nibble form may hand over utils.ConjSum halves
        for the folded renorm"""
        lut = self.sub if lut is None else lut
        defer = bool(defer_conj and FOLDS.conj and self.use_hard_renorm_between_steps and not self.true_fhe)
        return lut.apply(*ct, out_level=self._floor(), defer_conj=defer)

    def _packed_round_key(self, r: int):
        """round key r of the current schedule (after _prepare_round_keys) encrypted in the packed form, made once and
        kept on the schedule: clear key bytes are encoded packed, an encrypted key is packed homomorphically"""
        ks = self._schedule
        if ks.packed[r] is None:
            if ks.raw is not None:
                key = ks.raw[r]
                if self.states > 1 and key.shape == (16,):
                    key = np.broadcast_to(key, (self.states, 16))
                ks.packed[r] = self.encoder.encode_packed(key)
            elif self.use_hard_renorm_between_steps and not self.true_fhe:
                ks.packed[r] = self.encoder.renorm_pack(*ks.pairs[r])  # the packing renorm where it applies
            else:
                ks.packed[r] = self.encoder.pack(*ks.pairs[r])
        return ks.packed[r]

    def _fused_key(self, r: int, direction: int):
        """round key r of the current (clear) schedule permuted by ShiftRows (direction -1) / InvShiftRows (+1),
        encrypted once: the key of a SubBytes-AddRoundKey fusion across a ShiftRows (sub_bytes_ark.py)"""
        # only fuse_sub_ark calls this, and _check_encrypted_keys refuses an EncryptedRoundKeys (no raw, no fused) with
        # it, so the schedule here is always a ClearRoundKeys
        fused = self._schedule.fused
        if (r, direction) not in fused:
            fused[(r, direction)] = self._encode_key(shift_rows_bytes(self._schedule.raw[r], direction))
        return fused[(r, direction)]

    def _log_packed(self, dbg, tag: str, ct, **meta) -> None:
        """debug snapshot of a packed (hi | lo) state, decoded to bytes"""
        if dbg is None:
            return
        entry = {"ct_packed": ct, "meta": dict(meta, packed=True)}
        try:
            entry["plain"] = self.encoder.decode_packed(ct)
        except Exception as err:
            entry["plain"] = None
            entry["plain_err"] = repr(err)
        dbg[tag] = entry

    def _log_pair(self, dbg, tag: str, ct_hi, ct_lo, **meta) -> None:
        if dbg is None:
            return
        entry = {"ct_hi": ct_hi, "ct_lo": ct_lo, "meta": meta}
        try:
            entry["plain"] = self.encoder.decode(ct_hi, ct_lo)
        except Exception as err:  # keep the snapshot, record why decoding failed
            entry["plain"] = None
            entry["plain_err"] = repr(err)
        dbg[tag] = entry

    # ---------------------------------------------------------------- steps
    def add_round_key(self, ct_hi, ct_lo, key_hi, key_lo):
        return self.ark(ct_hi, ct_lo, key_hi, key_lo)

    def sub_bytes(self, ct_hi, ct_lo):
        return self.sub.apply(ct_hi, ct_lo)

    def inv_sub_bytes(self, ct_hi, ct_lo):
        if self.isub is None:
            raise KeyError("inv_sub_hi")
        return self.isub.apply(ct_hi, ct_lo)

    def shift_rows(self, ct_hi, ct_lo):
        return self.shift.apply(ct_hi, ct_lo)

    def inv_shift_rows(self, ct_hi, ct_lo):
        return self.invshift.apply(ct_hi, ct_lo)

    def mix_columns(self, ct_hi, ct_lo):
        return self.mix(ct_hi, ct_lo)

    def inv_mix_columns(self, ct_hi, ct_lo):
        return self.invmix(ct_hi, ct_lo)

    # ---------------------------------------------------------------- encrypt
    def encrypt_round(self, ct, key_pair, debug=None, r: int = 0, next_level: int | None = None):
        """One middle round r = 1..nr - 1 (nr = 10 / 12 / 14): SB, renorm, SR, MC, ARK, renorm (REF :142-151).  With a
        debug dict every step is logged under enc.r{r}.<step> (the names of the reference's
        one-round debug block, REF :154-171)."""
        if next_level is None:
            next_level = self.need_sub
        # a debug dict logs the stages of the path every call takes, under the reference's names: the levels, the
        # folds and the deferred conjugate (a utils.ConjSum is logged as it is, decoded if the encoder can) are
        # production's own
        ct = self._sub_apply(ct, defer_conj=True)
        self._log_pair(debug, f"enc.r{r}.sub", *ct)
        if self.packed_xor and r > 0:
            # packed XOR stage: MixColumns returns the packed state, AddRoundKey
            # XORs it with the packed round key, its renorm unpacks into the (hi, lo) pair (the packed
            # stages are logged decoded from the hi | lo halves)
            need = getattr(self.mix, "packed_input_need", None)
            lv = need() if need else NEED_SR_MIX - SHIFTROWS_DEPTH + self.encoder.PACK_DEPTH
            perm = self._fold_perm(self.shift, ct)
            entry = {}  # mix_packed's keywords when ShiftRows runs (and is logged) inside its entry
            if perm is not None:  # ShiftRows folded into the renorm (a byte permutation of the snap)
                ct = self.encoder.renorm_perm(*ct, perm, level=lv)
                self._log_pair(debug, f"enc.r{r}.sr", *ct)
            elif self._sr_entry_ok():
                # ShiftRows homomorphic inside MixColumns' entry (MixColFinal.sr_entry: masked rotations
                # fused with the first column shift and the packs, one level): the renorm hands out lv
                ct = self._renorm_pair(*ct, level=lv)
                self._log_pair(debug, f"enc.r{r}.sub.renorm", *ct)
                log_sr = (lambda p0: self._log_packed(debug, f"enc.r{r}.sr", p0)) if debug is not None else None
                entry = {"sr": self.shift, "on_sr": log_sr}
            else:
                ct = self._renorm_pair(*ct, level=lv + SHIFTROWS_DEPTH)
                self._log_pair(debug, f"enc.r{r}.sub.renorm", *ct)
                ct = self.shift_rows(*ct)
                self._log_pair(debug, f"enc.r{r}.sr", *ct)
            acc = self.mix.mix_packed(*ct, **entry)
            self._log_packed(debug, f"enc.r{r}.mc", acc)
            x = self._ark_packed(acc, r, defer_conj=True)
            self._log_packed(debug, f"enc.r{r}.ark", x)
            ct = self.encoder.renorm_unpack(x, level=next_level)
            self._log_pair(debug, f"enc.r{r}.ark.renorm", *ct)
            return ct
        ct = self._renorm_pair(*ct, level=self._sub_level(NEED_SR_MIX))
        self._log_pair(debug, f"enc.r{r}.sub.renorm", *ct)
        if self.srmc is not None:  # ShiftRows and MixColumns merged (shiftrows_mixcolumns.py)
            inner = {} if debug is not None else None  # the merged step's own ShiftRows output, only when logging
            ct = self.srmc(*ct, debug=inner)
            if inner is not None:
                self._log_pair(debug, f"enc.r{r}.sr", *inner["sr"])
        else:
            ct = self.shift_rows(*ct)
            self._log_pair(debug, f"enc.r{r}.sr", *ct)
            ct = self.mix_columns(*ct)
        self._log_pair(debug, f"enc.r{r}.mc", *ct)
        ct = self.ark(*ct, *key_pair, out_level=self._floor())
        self._log_pair(debug, f"enc.r{r}.ark", *ct)
        ct = self._renorm_pair(*ct, level=next_level)
        self._log_pair(debug, f"enc.r{r}.ark.renorm", *ct)
        return ct

    def encrypt(self, state: np.ndarray, round_keys: List[np.ndarray] | EncryptedRoundKeys, debug: Dict[str, Any] | None = None):
        """AES-128 / 192 / 256 by the number of round keys: 11 / 13 / 15 keys run 10 / 12 / 14 rounds"""
        round_count(round_keys)  # before the state is encrypted
        if debug is not None:
            debug.clear()
        ct = self.encoder.encode(state)
        self._log_pair(debug, "enc.input", *ct)
        rk = self._prepare_round_keys(round_keys)
        ct = self.ark(*ct, *rk[0], out_level=self._floor())
        return self._encrypt_tail(ct, rk, debug)

    def _encrypt_tail(self, ct, rk, debug):
        """encrypt after round 0's AddRoundKey: its renorm, rounds 1..nr - 1, the final round nr = len(rk) - 1 (shared
        by encrypt and encrypt_public, whose round 0 differs)"""
        nr = len(rk) - 1
        self._log_pair(debug, "enc.r0.ark", *ct)
        ct = self._renorm_pair(*ct, level=self.need_sub)
        self._log_pair(debug, "enc.r0.renorm", *ct)
        for r in range(1, nr):
            nxt = NEED_SUB_ARK_SR if (self.fuse_sub_ark and r == nr - 1) else self.need_sub
            ct = self.encrypt_round(ct, rk[r], debug, r, next_level=nxt)
        if self.fuse_sub_ark:
            # SR(SB(x)) ^ k_nr = SR(SB(x) ^ InvShiftRows(k_nr)): one fused LUT, then ShiftRows
            ct = self.sbark(*ct, *self._fused_key(nr, +1))
            self._log_pair(debug, "enc.final.sub_ark", *ct)
            ct = self.shift_rows(*ct)
        else:
            ct = self._sub_apply(ct, defer_conj=True)
            self._log_pair(debug, "enc.final.sub", *ct)
            perm = self._fold_perm(self.shift, ct)
            if perm is not None:  # ShiftRows folded into the renorm
                ct = self.encoder.renorm_perm(*ct, perm, level=NEED_SR_ARK - SHIFTROWS_DEPTH)
            else:
                ct = self._renorm_pair(*ct, level=NEED_SR_ARK)
                self._log_pair(debug, "enc.final.sub.renorm", *ct)
                ct = self.shift_rows(*ct)
            self._log_pair(debug, "enc.final.sr", *ct)
            ct = self.ark(*ct, *rk[nr], out_level=self._floor())
        self._log_pair(debug, f"enc.final.ark{nr}", *ct)
        ct = self._renorm_pair(*ct)
        self._log_pair(debug, "enc.output", *ct)
        return tag_layout(self.layout, *ct)

    # ---------------------------------------------------------------- public state / counter mode
    def _no_pairs(self, what: str) -> None:
        if self.pairs > 1:
            raise ValueError(f"{what}: multi-pair batches (pairs > 1) take no public operands")

    def encrypt_public(self, state: np.ndarray, round_keys: List[np.ndarray] | EncryptedRoundKeys, debug: Dict[str, Any] | None = None):
        """encrypt of a PUBLIC state (a counter block): round 0 XORs the encrypted round key 0 with the
        state's nibbles in clear (AddRoundKey.public; the state is never encrypted), everything after it is
        encrypt's own path.  Same bytes and the same layout-tagged pair as encrypt(state, round_keys); the
        debug stages keep encrypt's names (no "enc.input": there is no input ciphertext)."""
        self._no_pairs("encrypt_public")
        round_count(round_keys)  # 11 / 13 / 15 keys, checked before any GPU work
        if debug is not None:
            debug.clear()
        rk = self._prepare_round_keys(round_keys)
        ct = self.ark.public(*rk[0], *self.encoder.nibble_slots(state), out_level=self._floor())
        return self._encrypt_tail(ct, rk, debug)

    def ctr_keystream(self, nonce12, counter0: int, round_keys: List[np.ndarray] | EncryptedRoundKeys):
        """the encrypted keystream blocks of counters counter0 .. counter0 + states - 1 (mod 2^32) under the
        encrypted key: encrypt_public of ctr_mode.counter_blocks, one block per state"""
        from ctr_mode import counter_blocks
        self._no_pairs("ctr_keystream")
        round_count(round_keys)  # 11 / 13 / 15 keys, checked before any GPU work
        blocks = counter_blocks(nonce12, counter0, self.states)
        return self.encrypt_public(blocks[0] if self.states == 1 else blocks, round_keys)

    def transcipher(self, aes_ct: np.ndarray, nonce12, counter0: int, round_keys: List[np.ndarray] | EncryptedRoundKeys):
        """AES-CTR transciphering: aes_ct ((states, 16), or (16,) for one state) holds the client's
        m ^ keystream under this pipeline's cipher in counter mode (ctr_mode.ctr_xor); returns a clean
        layout-tagged pair that encoder.decode reads as m, at the level encrypt's output has.  The keystream
        is evaluated under the encrypted key and XORed with the public ciphertext bytes (AddRoundKey.public),
        then renormalised by the pipeline's own renorm (secret-key, or bootstrap + snap with true_fhe)."""
        self._no_pairs("transcipher")
        round_count(round_keys)  # 11 / 13 / 15 keys, checked before any GPU work
        nib = self.encoder.nibble_slots(aes_ct)  # checks the shape before any GPU work
        ks = self.ctr_keystream(nonce12, counter0, round_keys)
        ct = self.ark.public(*ks, *nib, out_level=self._floor())
        return tag_layout(self.layout, *self._renorm_pair(*ct))

    # ---------------------------------------------------------------- real-valued slots
    def _value_lut(self, gain: float):
        from xor_value_lut import XorValueLUT
        if getattr(self, "_value_luts", None) is None:
            self._value_luts = {}
        g = float(gain)
        if g not in self._value_luts:
            self._value_luts[g] = XorValueLUT(self.ctx, g)
        return self._value_luts[g]

    def _typed_lut(self, dtype, gain, offset):
        """None: today's path (unsigned bytes times one scalar gain, no offset: XorValueLUT, unchanged); else the
        TypedValueLUT of the value spec in this pipeline's layout and byte order"""
        from state_encoder import value_dtype
        w = value_dtype(dtype)[0]  # ValueError for anything but the six types
        if dtype == "u1" and (gain is None or np.ndim(gain) == 0) and np.ndim(offset) == 0 and float(offset) == 0.0:
            return None
        from xor_value_lut import TypedValueLUT
        return TypedValueLUT(self.ctx, self.encoder.value_slots((dtype, 256.0 ** -w if gain is None else gain, offset)))

    def transcipher_values(self, aes_ct: np.ndarray, nonce12, counter0: int, round_keys: List[np.ndarray] | EncryptedRoundKeys,
                           gain=None, dtype: str = "u1", offset=0.0):
        """AES-CTR transciphering to REAL-VALUED slots: transcipher's inputs, but the result is ONE layout-tagged
        ciphertext whose state slots hold gain * m as real numbers (in [0, 1) at the default gain; slots that hold
        no state hold 0) -- what a CKKS program can add, multiply or average, read back by encoder.decode_values.
        The keystream's last XOR (public AES ciphertext bytes) is fused with the value decode
        (xor_value_lut.XorValueLUT.apply_public): no XOR4, no renorm and no bootstrap come after the keystream, whose
        own last renorm (secret-key, or bootstrap + snap with true_fhe) is the last one.  The keystream is NOT
        dropped first: the output sits utils.XOR_VALUE_DEPTH = 4 levels below the keystream's fresh level (3 on the
        fresh-level-7 set, 13 on the default 17 / 5 set), and those levels are the caller's to compute with.

        Typed numbers, for no further level: dtype "u1" / "i1" (bytes) or "<u2" / ">u2" / "<i2" /
        ">i2" (16-bit words, w = 2 bytes, either byte order); gain and offset scalars or arrays broadcastable to
        (16 // w,) or (states, 16 // w) (gain None: 256^-w).  The slot of each word's first byte holds
        gain * q + offset, q the integer the message bytes spell in `dtype`; every other slot holds 0.
        decode_values returns (states, 16 // w).  dtype "u1" with a scalar gain and no offset is the path above,
        unchanged; any other dtype (32-bit words would add no precision over 16) raises ValueError."""
        out = _transcipher_with(self, "transcipher_values", aes_ct, nonce12, counter0, round_keys,
                                lambda: _values_lut(self, dtype, gain, offset))
        return tag_value_dtype(dtype, tag_layout(self.layout, out)[0])

    def to_values(self, ct_hi, ct_lo, gain=None, dtype: str = "u1", offset=0.0):
        """a clean layout-tagged (hi, lo) pair -- the output of encrypt, decrypt or transcipher -- as ONE ciphertext of
        gain * byte per state slot (XorValueLUT.apply; utils.XOR_VALUE_DEPTH levels below the pair); dtype, gain and
        offset as transcipher_values'"""
        out = _convert_with(self, "to_values", ct_hi, ct_lo, lambda: _values_lut(self, dtype, gain, offset))
        return tag_value_dtype(dtype, tag_layout(self.layout, out)[0])

    # ---------------------------------------------------------------- a linear map fused with the value decode
    def _linear_lut(self, weight, bias, dtype, in_scale, zero_point):
        from xor_value_lut import LinearValueLUT
        return LinearValueLUT(self.ctx, self.encoder.linear_slots(weight, bias, dtype, in_scale, zero_point))

    def transcipher_linear(self, aes_ct: np.ndarray, nonce12, counter0: int, round_keys: List[np.ndarray] | EncryptedRoundKeys, weight,
                           bias=0.0, dtype: str = "i1", in_scale=None, zero_point=0):
        """AES-CTR transciphering with a 16 x 16 LINEAR MAP over the bytes of every block fused into the value decode:
        transcipher_values' inputs and one layout-tagged output ciphertext, whose slot of byte position i of state b holds
            y[b, i] = sum_j weight[b, i, j] * (q[b, j] - zero_point[j]) * in_scale + bias[b, i],
        q the message bytes read as `dtype` ("u1" or "i1"; 16-bit types raise ValueError).  weight: (16, 16) or
        (states, 16, 16); bias broadcasts to (states, 16); in_scale a scalar (None: 1/256); zero_point a scalar or
        (16,).  A channel-mixing layer, a short FIR filter, a de-interleave or a dot product over a block costs no
        plaintext product and no level: the output sits utils.XOR_VALUE_DEPTH = 4 levels below the keystream, as
        transcipher_values' does (xor_value_lut.LinearValueLUT: the matrix's non-zero cyclic diagonals are weight
        groups of the decode, rotated together in one batched key switch).  Slots that hold no state hold 0;
        encoder.decode_values returns (states, 16)."""
        out = _transcipher_with(self, "transcipher_linear", aes_ct, nonce12, counter0, round_keys,
                                lambda: self._linear_lut(weight, bias, dtype, in_scale, zero_point))
        return tag_value_dtype(dtype, tag_layout(self.layout, out)[0])

    def to_linear(self, ct_hi, ct_lo, weight, bias=0.0, dtype: str = "i1", in_scale=None, zero_point=0):
        """a clean layout-tagged (hi, lo) pair as ONE ciphertext of weight (bytes - zero_point) * in_scale + bias per
        state (LinearValueLUT.apply; utils.XOR_VALUE_DEPTH levels below the pair); arguments as transcipher_linear's"""
        out = _convert_with(self, "to_linear", ct_hi, ct_lo, lambda: self._linear_lut(weight, bias, dtype, in_scale, zero_point))
        return tag_value_dtype(dtype, tag_layout(self.layout, out)[0])

    # ---------------------------------------------------------------- a 256-entry byte table fused with the value decode
    def _byte_lut(self, table, gain):
        from xor_value_lut import ByteValueLUT
        t = np.asarray(table, np.float64)
        if t.shape != (256,):
            raise ValueError(f"byte table: 256 reals, got shape {t.shape}")
        return ByteValueLUT(self.ctx, t, self.encoder.lut_slots(gain)[0])

    def transcipher_lut(self, aes_ct: np.ndarray, nonce12, counter0: int, round_keys: List[np.ndarray] | EncryptedRoundKeys, table,
                        gain=1.0):
        """AES-CTR transciphering through a 256-ENTRY TABLE of the message byte: transcipher_values' inputs and one
        layout-tagged output ciphertext whose slot of byte i of state b holds gain[b, i] * table[m[b, i]] -- ReLU or
        GELU of a quantised int8 activation, a G.711 sample, an sRGB pixel, an FP8 number, any 8-bit codebook; exact on
        the nibble code, where a polynomial of the decoded number would be deep and wrong at the kink.  table: 256
        finite reals indexed by the byte; gain: a scalar, or broadcastable to (16,) or (states, 16).  The output sits
        utils.BYTE_LUT_DEPTH = 5 levels below the keystream (one ct x ct level more than transcipher_values; 2 levels
        left on the fresh-level-7 set); no XOR4, renorm or bootstrap comes after the keystream
        (xor_value_lut.ByteValueLUT).  Slots that hold no state hold 0; encoder.decode_values returns (states, 16)."""
        out = _transcipher_with(self, "transcipher_lut", aes_ct, nonce12, counter0, round_keys, lambda: self._byte_lut(table, gain))
        return tag_value_dtype(LUT_VALUE_TAG, tag_layout(self.layout, out)[0])

    def to_lut(self, ct_hi, ct_lo, table, gain=1.0):
        """a clean layout-tagged (hi, lo) pair as ONE ciphertext of gain * table[byte] per state slot
        (ByteValueLUT.apply; utils.BYTE_LUT_DEPTH levels below the pair); table and gain as transcipher_lut's"""
        out = _convert_with(self, "to_lut", ct_hi, ct_lo, lambda: self._byte_lut(table, gain))
        return tag_value_dtype(LUT_VALUE_TAG, tag_layout(self.layout, out)[0])

    # ---------------------------------------------------------------- a bank of byte tables: a table per slot, several outputs
    def _byte_bank(self, tables, select, gain):
        from xor_value_lut import ByteValueBank, bank_coefficients
        t, _, c00s = bank_coefficients(tables)  # ValueError: not (T, 256) with 1 <= T <= 64, or a non-finite entry
        try:
            select = list(select)
        except TypeError:
            raise ValueError("byte table bank: select is a sequence of selectors, one per output") from None
        if not select:
            raise ValueError("byte table bank: select is empty (at least one output)")
        scalar = np.isscalar(gain) or (isinstance(gain, np.ndarray) and gain.ndim == 0)
        gains = [gain] * len(select) if scalar else list(gain)
        if len(gains) != len(select):
            raise ValueError(f"byte table bank: gain is one number or a sequence of {len(select)} (one per output), got {len(gains)}")
        return ByteValueBank(self.ctx, t, [self.encoder.lut_bank_slots(s, g, c00s) for s, g in zip(select, gains)])

    def _tag_bank(self, outs):
        return [tag_value_dtype(LUT_VALUE_TAG, tag_layout(self.layout, ct)[0]) for ct in outs]

    def transcipher_lut_bank(self, aes_ct: np.ndarray, nonce12, counter0: int, round_keys: List[np.ndarray] | EncryptedRoundKeys, tables,
                             select, gain=1.0):
        """transcipher_lut with a BANK of tables, a table per byte and SEVERAL OUTPUTS from one keystream: a list of K
        layout-tagged ciphertexts, output k's slot of byte i of state b holding
            gain_k[b, i] * tables[select[k][b, i]][m[b, i]]
        -- relu(q - zp_c) or clip(q - zp_c, lo_c, hi_c) with a zero point per channel, a codebook per field of a record,
        or several numbers of one byte (eight flag bits, two int4 values, (sin, cos) of a phase byte).  tables:
        (T, 256) finite reals, 1 <= T <= 64; select: a sequence of K >= 1 selectors, each integers in [0, T)
        broadcastable to (16,) or (states, 16); gain: one gain for all outputs (a scalar) or a sequence of K, each a
        scalar or broadcastable like a selector.  The keystream, the power bases and the seven conjugates are computed
        once for all outputs (xor_value_lut.ByteValueBank); every output sits utils.BYTE_LUT_DEPTH = 5 levels below the
        keystream, as transcipher_lut's.  Slots that hold no state hold 0; encoder.decode_values reads each output as
        (states, 16)."""
        return self._tag_bank(_transcipher_with(self, "transcipher_lut_bank", aes_ct, nonce12, counter0, round_keys,
                                                lambda: self._byte_bank(tables, select, gain)))

    def to_lut_bank(self, ct_hi, ct_lo, tables, select, gain=1.0):
        """a clean layout-tagged (hi, lo) pair as K ciphertexts of gain_k * tables[select[k]][byte] per state slot
        (ByteValueBank.apply; utils.BYTE_LUT_DEPTH levels below the pair); tables, select and gain as
        transcipher_lut_bank's"""
        return self._tag_bank(_convert_with(self, "to_lut_bank", ct_hi, ct_lo, lambda: self._byte_bank(tables, select, gain)))

    # ---------------------------------------------------------------- decrypt
    def decrypt(self, ct_hi, ct_lo, round_keys: List[np.ndarray] | EncryptedRoundKeys, debug: Dict[str, Any] | None = None):
        """the inverse of encrypt: 11 / 13 / 15 round keys undo 10 / 12 / 14 rounds"""
        nr = round_count(round_keys)
        check_layout(self.layout, ct_hi, ct_lo)  # a pair from another layout would decrypt to wrong bytes
        if debug is not None:
            debug.clear()
        rk = self._prepare_round_keys(round_keys)
        self._log_pair(debug, "dec.input", ct_hi, ct_lo)
        if self.true_fhe and not self.fuse_sub_ark:
            return self._decrypt_fhe(ct_hi, ct_lo, rk, debug)
        ct = self.ark(ct_hi, ct_lo, *rk[nr], out_level=self._floor())
        self._log_pair(debug, f"dec.init.ark{nr}", *ct)
        fuse = self.fuse_sub_ark
        if fuse and self.isub is None:
            raise KeyError("inv_sub_hi")
        # InvShiftRows folded into the renorm before it (the packed decrypt: this renorm and every
        # InvMixColumns renorm), as ShiftRows in encrypt
        isr = self._fold_perm(self.invshift, ct) if self.packed_dec and not fuse else None
        if isr is not None:
            ct, isr_done = self.encoder.renorm_perm(*ct, isr, level=self.need_isr_isb - SHIFTROWS_DEPTH), True
        else:
            ct, isr_done = self._renorm_pair(*ct, level=NEED_SUB_ARK_SR if fuse else self.need_isr_isb), False
        self._log_pair(debug, f"dec.init.ark{nr}.renorm", *ct)
        for r in range(nr - 1, 0, -1):
            if fuse:
                # ISB(ISR(x)) ^ k_r = ISR(ISB(x) ^ ShiftRows(k_r)): one fused LUT, then InvShiftRows
                ct = self.isbark(*ct, *self._fused_key(r, -1))
                self._log_pair(debug, f"dec.r{r}.isb_ark", *ct)
                ct = self.inv_shift_rows(*ct)
                ct = self._renorm_pair(*ct, level=NEED_GF if self.with_inv_mix_columns else NEED_SUB_ARK_SR)
                self._log_pair(debug, f"dec.r{r}.ark", *ct)
                if self.with_inv_mix_columns:
                    ct = self._renorm_pair(*self.inv_mix_columns(*ct), level=NEED_SUB_ARK_SR)
                    self._log_pair(debug, f"dec.r{r}.imc", *ct)
                continue
            if self.packed_dec:
                # packed XOR stage: AddRoundKey on the packed state, its renorm
                # unpacking; InvMixColumns' XOR stage packed, unpacked by the renorm after it
                # (a debug dict logs this path's stages under the reference's names)
                if not isr_done:
                    ct = self.inv_shift_rows(*ct)
                isr_done = False
                self._log_pair(debug, f"dec.r{r}.isr", *ct)
                ct = self._sub_renorm(ct, inverse=True, level=NEED_XOR + self.encoder.PACK_DEPTH)
                self._log_pair(debug, f"dec.r{r}.isb", *ct)
                x = self._ark_packed(self.encoder.pack(*ct), r, defer_conj=True)
                need = getattr(self.invmix, "packed_input_need", None)
                ct = self.encoder.renorm_unpack(x, level=need() if need else NEED_GF + self.encoder.PACK_DEPTH)
                self._log_pair(debug, f"dec.r{r}.ark", *ct)
                if isr is not None:
                    ct = self.encoder.renorm_unpack_perm(self.invmix.imc_packed(*ct), isr, level=self.need_isr_isb - SHIFTROWS_DEPTH)
                    isr_done = True
                else:
                    ct = self.encoder.renorm_unpack(self.invmix.imc_packed(*ct), level=self.need_isr_isb)
                self._log_pair(debug, f"dec.r{r}.imc", *ct)
                continue
            ct = self.inv_shift_rows(*ct)
            self._log_pair(debug, f"dec.r{r}.isr", *ct)
            ct = self._sub_renorm(ct, inverse=True, level=NEED_XOR)
            self._log_pair(debug, f"dec.r{r}.isb", *ct)
            ct = self._ark_renorm(ct, rk[r], level=NEED_GF if self.with_inv_mix_columns else self.need_isr_isb)
            self._log_pair(debug, f"dec.r{r}.ark", *ct)
            if self.with_inv_mix_columns:
                # InvSubBytes' LUT needs a clean input, as SubBytes gets one after ARK in encrypt
                ct = self._renorm_pair(*self.inv_mix_columns(*ct), level=self.need_isr_isb)
                self._log_pair(debug, f"dec.r{r}.imc", *ct)
        if fuse:
            ct = self.isbark(*ct, *self._fused_key(0, -1))
            self._log_pair(debug, "dec.final.isb_ark", *ct)
            ct = self.inv_shift_rows(*ct)
        else:
            if not isr_done:
                ct = self.inv_shift_rows(*ct)
            self._log_pair(debug, "dec.final.isr", *ct)
            if self.isub is None:
                raise KeyError("inv_sub_hi")
            ct = self.isub.apply(*ct, out_level=self._floor())
            self._log_pair(debug, "dec.final.isb", *ct)
            ct = self._renorm_pair(*ct, level=NEED_XOR)
            self._log_pair(debug, "dec.final.isb.renorm", *ct)
            ct = self.ark(*ct, *rk[0], out_level=self._floor())
        self._log_pair(debug, "dec.final.ark0", *ct)
        ct = self._renorm_pair(*ct)
        self._log_pair(debug, "dec.output", *ct)
        return ct

    def _decrypt_fhe(self, ct_hi, ct_lo, rk, debug):
        """decrypt in true-FHE mode: the same steps, each InvShiftRows applied BEFORE the renorm
        (bootstrap + snap) that precedes InvSubBytes -- after the snap exactly InvSubBytes' 13
        levels remain.  InvShiftRows is a masked permutation, so moving it across the renorm
        changes no byte (ISB(ISR(x)) with x renormalised either side)."""
        if self.isub is None:
            raise KeyError("inv_sub_hi")
        fl = self._floor()
        nr = len(rk) - 1
        ct = self.ark(ct_hi, ct_lo, *rk[nr], out_level=fl)
        self._log_pair(debug, f"dec.init.ark{nr}", *ct)
        ct = self._renorm_pair(*self.inv_shift_rows(*ct), level=NEED_SUBBYTES)
        self._log_pair(debug, f"dec.r{nr - 1}.isr", *ct)
        for r in range(nr - 1, -1, -1):
            # InvSubBytes' output error is ~3e-2: its renorm snaps twice before AddRoundKey's XOR4
            ct = self._renorm_pair(*self.isub.apply(*ct, out_level=fl), level=NEED_XOR)
            self._log_pair(debug, f"dec.r{r}.isb" if r else "dec.final.isb.renorm", *ct)
            ct = self.ark(*ct, *rk[r], out_level=fl)
            if r == 0:
                self._log_pair(debug, "dec.final.ark0", *ct)
                ct = self._renorm_pair(*ct)
                self._log_pair(debug, "dec.output", *ct)
                return ct
            if self.with_inv_mix_columns:
                ct = self._renorm_pair(*ct, level=NEED_GF)
                self._log_pair(debug, f"dec.r{r}.ark", *ct)
                ct = self.invmix(*ct, final_renorm=False)
            ct = self._renorm_pair(*self.inv_shift_rows(*ct), level=NEED_SUBBYTES)
            self._log_pair(debug, f"dec.r{r}.imc" if self.with_inv_mix_columns else f"dec.r{r}.ark", *ct)
