"""Counter mode over a 16-byte block function: plain byte helpers, no engine.

The block function is whatever the caller passes: fips_block_fn(rks) is FIPS-197 AES-128, the cipher of
AESPipeline(fips=True), and makes ctr_xor the standard AES-CTR of NIST SP 800-38A (its 16-byte initial counter
block split into nonce12 and a 32-bit counter); the default pipeline computes the reference's cipher instead
(oracle/aes_plain.ref_encrypt: its MixColumns mixes along rows).  Nothing here looks inside a block:
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


def fips_block_fn(rks):
    """FIPS-197 AES-128 encryption under the 11 round keys rks as a block function for ctr_xor: the standard
    AES-CTR (SP 800-38A) whose ciphertexts AESPipeline(fips=True).transcipher inverts.  Plain bytes, column-first
    state (byte r + 4c), MixColumns along the columns as the standard has it"""
    from aes_keyschedule import SBOX
    from shift_rows import shift_rows_bytes
    keys = [np.asarray(k, dtype=np.uint8).reshape(16) for k in rks]
    if len(keys) != 11:
        raise ValueError("AES-128 takes 11 round keys")

    def xtime(a):
        return (((a.astype(np.uint16) << 1) ^ np.where(a & 0x80, 0x1B, 0)) & 0xFF).astype(np.uint8)

    def mix_columns(s):
        a = s.reshape(4, 4)  # [c, r]
        out = np.empty_like(a)
        for r in range(4):
            x, y = a[:, r], a[:, (r + 1) % 4]
            out[:, r] = xtime(x) ^ xtime(y) ^ y ^ a[:, (r + 2) % 4] ^ a[:, (r + 3) % 4]
        return out.reshape(16)

    def block(pt):
        s = np.asarray(pt, dtype=np.uint8).reshape(16) ^ keys[0]
        for r in range(1, 10):
            s = mix_columns(shift_rows_bytes(SBOX[s], -1)) ^ keys[r]
        return shift_rows_bytes(SBOX[s], -1) ^ keys[10]

    return block


def ctr_xor(block_fn, data, nonce12, counter0: int) -> np.ndarray:
    """data (n, 16) XOR the keystream block_fn(counter block i): encryption and decryption alike (the
    byte model of AESPipeline.transcipher's input and of its tests)"""
    data = np.asarray(data, dtype=np.uint8)
    if data.ndim != 2 or data.shape[1] != 16:
        raise ValueError("data: an (n, 16) uint8 array of blocks")
    ks = np.stack([np.asarray(block_fn(b), dtype=np.uint8) for b in counter_blocks(nonce12, counter0, data.shape[0])]) \
        if data.shape[0] else np.zeros((0, 16), np.uint8)
    return data ^ ks
