"""Counter mode over a 16-byte block function: plain byte helpers, no engine.

The block function is whatever the caller passes: fips_block_fn(rks) is FIPS-197 AES-128 / 192 / 256 by the number of
round keys (11 / 13 / 15), the cipher of AESPipeline(fips=True), and makes ctr_xor the standard AES-CTR of NIST SP 800-38A
(its 16-byte initial counter block split into nonce12 and a 32-bit counter); the default pipeline computes the
reference's cipher instead, ref_block_fn(rks) (its MixColumns mixes along rows; on 11 round keys it is
oracle/aes_plain.ref_encrypt).  Nothing here looks inside a block:
a counter block is 16 bytes handed to the block function as they are, and the keystream is XORed byte
for byte, so another byte order inside the block function changes nothing in this module.
"""
from __future__ import annotations

import numpy as np


def counter_blocks(nonce12, counter0: int, n: int) -> np.ndarray:
    """(n, 16) uint8: block i = nonce12 || be32((counter0 + i) mod 2^32)"""
    nonce = np.frombuffer(bytes(nonce12), dtype=np.uint8) if isinstance(nonce12, (bytes, bytearray)) else np.asarray(nonce12, dtype=np.uint8)
    if nonce.shape != (12,):
        raise ValueError("the nonce is 12 bytes")
    if n < 0 or not 0 <= int(counter0) < 1 << 32:
        raise ValueError("counter0 must lie in [0, 2^32) and n be >= 0")
    ctr = (int(counter0) + np.arange(n, dtype=np.uint64)) % np.uint64(1 << 32)
    out = np.empty((n, 16), dtype=np.uint8)
    out[:, :12] = nonce
    for k in range(4):
        out[:, 12 + k] = (ctr >> np.uint64(8 * (3 - k))) & np.uint64(0xFF)
    return out


ROUND_KEY_COUNTS = (11, 13, 15)  # AES-128 / 192 / 256: Nr + 1 round keys


def _round_keys(rks):
    keys = [np.asarray(k, dtype=np.uint8).reshape(16) for k in rks]
    if len(keys) not in ROUND_KEY_COUNTS:
        raise ValueError(f"AES takes 11 round keys (AES-128), 13 (AES-192) or 15 (AES-256), got {len(keys)}")
    return keys


def _xtime(a):
    return (((a.astype(np.uint16) << 1) ^ np.where(a & 0x80, 0x1B, 0)) & 0xFF).astype(np.uint8)


def _mix(s, axis: int):
    """MixColumns on a column-first state seen as a[c, r]: axis 1 mixes the rows of a column (FIPS-197), axis 0 the
    columns of a row (the reference's orientation): out = 2 a ^ 3 a(+1) ^ a(+2) ^ a(+3) along `axis`"""
    a = s.reshape(4, 4)
    y = np.roll(a, -1, axis=axis)
    return (_xtime(a) ^ _xtime(y) ^ y ^ np.roll(a, -2, axis=axis) ^ np.roll(a, -3, axis=axis)).reshape(16)


def _block_fn(rks, axis: int):
    from aes_keyschedule import SBOX
    from shift_rows import shift_rows_bytes
    keys = _round_keys(rks)
    nr = len(keys) - 1

    def block(pt):
        s = np.asarray(pt, dtype=np.uint8).reshape(16) ^ keys[0]
        for r in range(1, nr):
            s = _mix(shift_rows_bytes(SBOX[s], -1), axis) ^ keys[r]
        return shift_rows_bytes(SBOX[s], -1) ^ keys[nr]

    return block


def fips_block_fn(rks):
    """FIPS-197 AES encryption under the 11, 13 or 15 round keys rks (AES-128 / 192 / 256: len(rks) - 1 rounds) as a
    block function for ctr_xor: the standard AES-CTR (SP 800-38A) whose ciphertexts
    AESPipeline(fips=True).transcipher inverts.  Plain bytes, column-first state (byte r + 4c), MixColumns along the
    columns as the standard has it"""
    return _block_fn(rks, 1)


def ref_block_fn(rks):
    """the cipher of the default AESPipeline (no fips) under 11, 13 or 15 round keys: FIPS-197's round sequence with
    the reference's MixColumns, which mixes along the rows of the column-first state -- the byte
    model of its encrypt, ctr_keystream and transcipher at every key size"""
    return _block_fn(rks, 0)


def ctr_xor(block_fn, data, nonce12, counter0: int) -> np.ndarray:
    """data (n, 16) XOR the keystream block_fn(counter block i): encryption and decryption alike (the
    byte model of AESPipeline.transcipher's input and of its tests)"""
    data = np.asarray(data, dtype=np.uint8)
    if data.ndim != 2 or data.shape[1] != 16:
        raise ValueError("data: an (n, 16) uint8 array of blocks")
    ks = np.stack([np.asarray(block_fn(b), dtype=np.uint8) for b in counter_blocks(nonce12, counter0, data.shape[0])]) \
        if data.shape[0] else np.zeros((0, 16), np.uint8)
    return data ^ ks
