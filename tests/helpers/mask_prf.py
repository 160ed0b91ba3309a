"""The engine's counter-mode PRF (csrc/common.h chacha_u64) vectorised in numpy: ChaCha20, 20 rounds on
uint32 arrays, 64-bit block counter and 64-bit nonce, the first 64 bits of the block.  One block per counter, so a
whole polynomial -- or a whole key -- is one call.

tests/test_compressed_keys.py pins it against the oracle's block function; tests/test_gpu_compressed_keys.py uses it
as the model of the `a` halves a mask key generates: uniform_rows is k_sample_uniform's value."""
import numpy as np

_SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def key_words(key) -> np.ndarray:
    """the 8 little-endian uint32 words of a 32-byte key (aesfhe_create_keyed, aesfhe_set_mask_key); 8 words pass through"""
    if isinstance(key, (bytes, bytearray)):
        if len(key) != 32:
            raise ValueError("a key is 32 bytes")
        return np.frombuffer(bytes(key), "<u4").astype(np.uint32)
    w = np.asarray(key, np.uint32)
    if w.shape != (8,):
        raise ValueError("a key is 8 words")
    return w


def stream_id(kind: int, a: int = 0, b: int = 0) -> int:
    """csrc/engine.hip stream_id: what is sampled (kind), for which key tag (a), which digit or level (b)"""
    return ((int(kind) << 56) | (int(a) << 16) | int(b)) & 0xFFFFFFFFFFFFFFFF


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def _qr(x, a, b, c, d):
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 16)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 12)
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 8)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 7)


def chacha_u64(key, stream, ctr) -> np.ndarray:
    """first 64 bits of the ChaCha20 block (key, counter ctr, nonce stream); ctr and stream broadcast, uint64 out"""
    kw = key_words(key)
    ctr, stream = np.broadcast_arrays(np.asarray(ctr, np.uint64), np.asarray(stream, np.uint64))
    shape = ctr.shape
    lo32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    init = [np.full(shape, w, np.uint32) for w in _SIGMA] + [np.full(shape, w, np.uint32) for w in kw]
    init += [(ctr & lo32).astype(np.uint32), (ctr >> s32).astype(np.uint32),
             (stream & lo32).astype(np.uint32), (stream >> s32).astype(np.uint32)]
    x = [w.copy() for w in init]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
            _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
        w0, w1 = x[0] + init[0], x[1] + init[1]
    return w0.astype(np.uint64) | (w1.astype(np.uint64) << s32)


def uniform_rows(key, stream, primes, moduli, log_n: int) -> np.ndarray:
    """[len(primes)][N] uint32: row i is the uniform polynomial of prime index primes[i] (k_sample_uniform:
    prf(key, stream, (prime << log_n) + k) mod q_prime); stream: one id, or one per row"""
    primes = np.asarray(primes, np.uint64).reshape(-1, 1)
    q = np.asarray(moduli, np.uint64)[primes.astype(np.int64)]
    k = np.arange(1 << log_n, dtype=np.uint64).reshape(1, -1)
    stream = np.asarray(stream, np.uint64).reshape(-1, 1)
    return (chacha_u64(key, stream, (primes << np.uint64(log_n)) + k) % q).astype(np.uint32)
