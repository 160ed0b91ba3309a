"""Seeded symmetric encryption: a client that holds the secret encrypts as c = (e + m - a s, a) with `a`
the PRF under the public mask key, ships the `b` rows plus a 56-bit id, and any context holding the mask key -- an
evaluation-only server above all -- regenerates `a` on its device (k_sym_encrypt, k_complete_ct).

Everything but the decryption error is exact, word for word: the `a` rows and the error polynomials against the numpy
ChaCha20 of tests/helpers/mask_prf.py, the server's ciphertexts and results against the client's.  Sets: RAW and BOOT
of tests/test_gpu_compressed_keys.py at N = 2^13, and once the 11 / 4 set at N = 2^16.
"""
import ctypes
import gc
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

pytestmark = pytest.mark.gpu

RAW = dict(log_n=13, max_level=6, dnum=3, allow_insecure=True)
BOOT = dict(log_n=13, use_bootstrap=True, max_level=3, dnum=5, allow_insecure=True)
SETS = {"raw": (RAW, 0xE7A1), "boot": (BOOT, 7)}   # parameters, seed (= encryption nonce unless a test says otherwise)
MASK = bytes(range(0xA0, 0xC0))
K_ENC_MAX = 16384   # csrc/kernels.h kEncMax


def _engine(which, mask_key=MASK, enc_nonce=None):
    from mi355x_ckks import Engine
    params, seed = SETS[which]
    return Engine(seed=seed, enc_nonce=seed if enc_nonce is None else enc_nonce, mask_key=mask_key, **params)


def _context(which, mask_key=MASK):
    from engine_context import EngineContext
    params, seed = SETS[which]
    p = dict(params)
    if p.pop("use_bootstrap", False):
        return EngineContext(signature=1, boot_fresh_level=p.pop("max_level"), seed=seed, enc_nonce=seed, mask_key=mask_key, **p)
    return EngineContext(signature=2, seed=seed, enc_nonce=seed, mask_key=mask_key, **p)


def _server(C):
    from engine_context import EngineContext
    return EngineContext.from_evaluation_keys(C.export_evaluation_keys(compressed=True), allow_insecure=True)


def _unit(E, seed, count):
    rng = np.random.default_rng(seed)
    return [np.exp(2j * np.pi * rng.random(E.slot_count)) for _ in range(count)]


def _enc_key(seed: int, nonce: int) -> np.ndarray:
    """Engine::enc_key of an int-seeded context: the seed in key words 0-1, the nonce folded into words 6-7"""
    w = np.zeros(8, np.uint32)
    w[0], w[1] = seed & 0xFFFFFFFF, seed >> 32
    w[6] ^= np.uint32(nonce & 0xFFFFFFFF)
    w[7] ^= np.uint32(nonce >> 32)
    return w


def _pop21(x):
    return sum(((x >> np.uint64(i)) & np.uint64(1)).astype(np.int64) for i in range(21))


def _binomial(key, stream, n) -> np.ndarray:
    """k_sample_small's kind 1: popcount of bits 0..20 minus popcount of bits 21..41 of the PRF word, |e| <= 21"""
    from mask_prf import chacha_u64
    r = chacha_u64(key, stream, np.arange(n, dtype=np.uint64))
    return _pop21(r) - _pop21(r >> np.uint64(21))


def _a_rows(E, ct, nonce16=None):
    from mask_prf import stream_id, uniform_rows
    sid = ct.seed_id
    assert sid is not None and (sid & 0xFFFF) == (E.enc_nonce & 0xFFFF if nonce16 is None else nonce16)
    return uniform_rows(MASK, stream_id(12, sid >> 16, sid & 0xFFFF), range(E.nl(ct.level)), E.moduli(), E.log_n)


@pytest.fixture(scope="module", params=list(SETS))
def client(request):
    """(set name, mask-key EngineContext) shared by the tests that need no fresh counter"""
    return request.param, _context(request.param)


# ---------------------------------------------------------------- 1. a is the PRF
@pytest.mark.parametrize("which", list(SETS))
def test_a_is_the_prf_and_the_counter_continues(which):
    E = _engine(which)
    z = _unit(E, 1, 3)
    n16 = E.enc_nonce & 0xFFFF
    first = E.encrypt_seeded_many(z)                       # B = 3: counters 0, 1, 2
    one = E.encrypt_seeded(z[0])                           # B = 1: counter 3
    low = E.encrypt_seeded_many(z, level=1)                # level 1: counters 4, 5, 6
    assert [c.seed_id for c in first + [one] + low] == [(j << 16) | n16 for j in range(7)]
    assert [c.level for c in first + [one] + low] == [E.fresh_level] * 4 + [1] * 3
    for c in first + [one] + low:
        x = E.export(c)
        assert x.shape == (2, E.nl(c.level), E.n)
        assert np.array_equal(x[1], _a_rows(E, c)), hex(c.seed_id)
        assert not np.array_equal(x[0], x[1])
    # another encryption nonce (its low 16 bits differ): another a at the same counter, the PRF at ITS id
    F = _engine(which, enc_nonce=SETS[which][1] + 1)
    f0 = F.encrypt_seeded(z[0])
    assert f0.seed_id >> 16 == 0 and f0.seed_id != first[0].seed_id
    assert np.array_equal(F.export(f0)[1], _a_rows(F, f0, (SETS[which][1] + 1) & 0xFFFF))
    assert not np.array_equal(F.export(f0)[1], E.export(first[0])[1])


# ---------------------------------------------------------------- 2. the ciphertext is exactly m + e
def _phase_coeffs(E, ct, s):
    """d = b + a s (mod q per limb) of a ciphertext, in coefficient form: the encoded message plus e"""
    x = E.export(ct).astype(np.uint64)
    nl = x.shape[1]
    q = E.moduli().astype(np.uint64)[:nl].reshape(-1, 1)
    d = (x[0] + x[1] * s[:nl].astype(np.uint64) % q) % q
    return E.debug_ntt(d.astype(np.uint32), 0, inverse=True).astype(np.int64), q.astype(np.int64)


@pytest.mark.parametrize("which", list(SETS))
def test_the_phase_is_message_plus_e(which):
    from mask_prf import stream_id
    E = _engine(which)
    seed = SETS[which][1]
    ek = _enc_key(seed, E.enc_nonce)
    s = E.export_secret()
    z = _unit(E, 2, 1)[0]
    for level in (None, 1):
        cts = E.encrypt_seeded_many([z, z, z], level)      # B = 3: one message under three ids
        cts.append(E.encrypt_seeded(z, level))             # B = 1: and a fourth
        ds, q = zip(*[_phase_coeffs(E, c, s) for c in cts])
        es = [_binomial(ek, stream_id(13, c.seed_id >> 16, c.seed_id & 0xFFFF), E.n) for c in cts]
        assert all(np.abs(e).max() <= 21 and np.abs(e).max() > 0 for e in es)
        for j in range(1, len(cts)):
            diff = (ds[0] - ds[j]) % q[0]
            diff = np.where(diff > q[0] // 2, diff - q[0], diff)             # centred, every limb
            want = np.broadcast_to(es[0] - es[j], diff.shape)
            assert np.array_equal(diff, want), (level, j)
            assert np.abs(diff).max() <= 42


@pytest.mark.parametrize("which", list(SETS))
def test_decrypt_against_public_key_encryption(which):
    """Slot error of a seeded encryption against a public-key encryption of the same data, measured here.

    The bound is HALF the reference's error.  Both share the encoder's rounding (uniform in [-1/2, 1/2] per
    coefficient, variance 1/12).  The seeded ciphertext adds e alone: centred binomial of 2 x 21 bits, variance 10.5,
    sigma 3.3 with the rounding.  The public-key one is rescaled from one limb above, which leaves (v e_pk + e0 + e1 s)
    / q_top (far below 1) plus the rescale's rounding r0 + r1 s, r uniform in [-1/2, 1/2] and s ternary of about 2N / 3
    non-zero coefficients: variance (1 + 2N / 3) / 12 = 455 at N = 2^13, sigma 21.3.  The expected ratio of the two
    errors is 3.3 / 21.3 = 0.15; the maxima over N / 2 slots of two independent draws differ from that by a few tens
    of per cent at most, so 0.5 leaves a factor of about three.  At level 1 the same bound is scaled by
    delta_fresh / delta_1, the slot error being noise / delta."""
    E = _engine(which)
    z = _unit(E, 3, 3)
    ref = max(np.abs(E.decrypt(E.encrypt(v)) - v).max() for v in z)
    delta = E.scales()
    for level in (E.fresh_level, 1):
        cts = E.encrypt_seeded_many(z, level) + [E.encrypt_seeded(z[0], level)]
        err = max(np.abs(E.decrypt(c) - v).max() for c, v in zip(cts, z + [z[0]]))
        bound = 0.5 * ref * delta[E.fresh_level] / delta[level]
        print(f"{which} level {level}: seeded max slot error {err:.3g}, public-key {ref:.3g} (fresh level), bound {bound:.3g}")
        assert err < bound


# ---------------------------------------------------------------- 3. the wire
def _ops(E, a, b):
    """a product with its relinearisation, and a rotation of it"""
    r = E._raw_mul(a, b, True)
    E.settle(r)
    return [E.export(r), E.export(E.rotate(r, delta=1)), E.export(E.rotate(a, delta=1))]


def test_halves_cross_the_wire_word_for_word(client):
    from state_encoder import StateEncoder, dump_ct, dump_ct_seeded, load_ct, load_ct_seeded, load_cts_seeded
    which, C = client
    E = C.engine
    z = _unit(E, 4, 3)
    cts = C.encrypt_seeded_many(z)                           # B = 3 at the fresh level
    low = C.encrypt_seeded(z[0], level=1)                    # B = 1 at level 1
    want = _ops(E, cts[0], cts[1])                           # also the warm-up: the keys exist from here on
    want_low = E.export(E.rotate(low, delta=1))
    S = _server(C)
    V = S.engine
    assert not V.has_secret and V.mask_key() == MASK
    recs = [dump_ct_seeded(C, c) for c in cts]
    for (b, level, tag, sid), c in zip(recs, cts):
        full = E.export(c)
        assert b.dtype == np.uint32 and 2 * b.nbytes == full.nbytes and np.array_equal(b, full[0])
        assert (level, tag, sid) == (E.fresh_level, None, c.seed_id)
    got = load_cts_seeded(S, recs)                           # one batched import of three consecutive ids
    for g, c in zip(got, cts):
        assert g.level == c.level and np.array_equal(V.export(g), E.export(c))
    b, level, tag, sid = dump_ct_seeded(C, low)
    slow = load_ct_seeded(S, b, level, sid, tag)             # B = 1, level 1
    assert slow.level == 1 and np.array_equal(V.export(slow), E.export(low))
    for x, y in zip(_ops(V, got[0], got[1]), want):
        assert np.array_equal(x, y)
    assert np.array_equal(V.export(V.rotate(slow, delta=1)), want_low)
    # a state pair keeps its layout tag and decodes to its bytes
    enc = StateEncoder(C)
    state = np.random.default_rng(5).integers(0, 256, 16).astype(np.uint8)
    pair = enc.encode(state, seeded=True)
    assert pair[1].seed_id == pair[0].seed_id + (1 << 16)
    prec = [dump_ct_seeded(C, c) for c in pair]
    assert all(r[2] is not None and r[2]["sc"] == E.slot_count for r in prec)
    spair = load_cts_seeded(S, prec)
    assert all(enc.layout.same(c.layout) for c in spair)
    back = [load_ct(C, *dump_ct(S, c)) for c in spair]       # the server cannot decrypt: back as whole ciphertexts
    assert np.array_equal(enc.decode(*back), state) and np.array_equal(enc.decode(*pair), state)


# ---------------------------------------------------------------- 4. refusals
def _raw_encrypt(E, count, level=-1):
    re = np.zeros(E.slot_count)
    out = (ctypes.c_uint64 * 1)()
    E._ctx.check(E._lib.aesfhe_encrypt_sym(E._ctx.ptr, re, re, count, level, out, None))


def _raw_import(E, count, level):
    d = np.zeros(E.n, np.uint32)
    out = (ctypes.c_uint64 * 1)()
    rows = (ctypes.c_void_p * 1)(d.ctypes.data)
    E._ctx.check(E._lib.aesfhe_import_half(E._ctx.ptr, rows, d.size, level, 0, count, out))


def test_refusals_leave_the_context_usable(client):
    from state_encoder import dump_ct_seeded
    which, C = client
    E = C.engine
    fresh, n = E.fresh_level, E.n
    q = [int(m) for m in E.moduli()]
    z = _unit(E, 6, 3)
    cts = C.encrypt_seeded_many(z)
    E.export(E.rotate(cts[0], delta=1))                      # a key for the bundle
    S = _server(C)
    V = S.engine
    halves = np.stack([E.export_half(c)[0] for c in cts])
    id0 = cts[0].seed_id

    def covered_server():
        got = V.import_half_many(halves, fresh, id0)
        assert all(np.array_equal(V.export(g), E.export(c)) for g, c in zip(got, cts))
        V.export(V.rotate(got[0], delta=1))

    def covered_client():
        c = E.encrypt_seeded_many(z)
        assert np.abs(E.decrypt(c[2]) - z[2]).max() < 2e-4
        # the successful halves of the refused calls below (a sum, a public-key encryption): the pool has their
        # buffers before it is measured, so only a buffer a refusal kept could make it grow
        E.export(E._raw_add(c[0], c[1])), E.export(C.add(c[0], c[1])), E.export(C.encrypt(z[0]))

    covered_server(), covered_client()
    V.sync(), E.sync()
    before_v, before_e = V.pool_stats()["bytes"], E.pool_stats()["bytes"]
    # --- the client side
    D = _engine(which, mask_key=None)                        # keyed, no mask key
    with pytest.raises(RuntimeError, match="a drawn under the context key cannot be published"):
        D.encrypt_seeded(z[0])
    with pytest.raises(RuntimeError, match="no secret key"):
        S.encrypt_seeded(z[0])
    for level in (fresh + 1, -2):
        with pytest.raises(RuntimeError, match="level out of range"):
            _raw_encrypt(E, 1, level)
    for count in (0, -1, K_ENC_MAX + 1):
        with pytest.raises(RuntimeError, match=rf"batch size outside 1\.\.{K_ENC_MAX}"):
            _raw_encrypt(E, count)
    with pytest.raises(RuntimeError, match="not a seeded ciphertext"):
        dump_ct_seeded(C, E._raw_add(cts[0], cts[1]))        # a sum of two seeded ciphertexts
    with pytest.raises(RuntimeError, match="not a seeded ciphertext"):
        dump_ct_seeded(C, C.add(cts[0], cts[1]))
    with pytest.raises(RuntimeError, match="not a seeded ciphertext"):
        dump_ct_seeded(C, C.encrypt(z[0]))                   # a public-key ciphertext
    with pytest.raises(RuntimeError, match="not a seeded ciphertext"):
        dump_ct_seeded(S, V.import_half(halves[0], fresh, id0))   # an import carries no id either
    # --- the server side
    from mi355x_ckks import Engine
    U = Engine.evaluation_only(enc_nonce=1, **SETS[which][0])   # evaluation-only, no mask key
    with pytest.raises(RuntimeError, match="no mask key"):
        U.import_half(halves[0], fresh, id0)
    with pytest.raises(RuntimeError, match="no mask key"):
        D.import_half(halves[0], fresh, id0)
    with pytest.raises(RuntimeError, match="word count"):
        V.import_half_many(halves[:, :-1], fresh, id0)       # a limb short
    with pytest.raises(RuntimeError, match="word count"):
        V.import_half_many(np.stack([E.export(c) for c in cts]).reshape(3, -1, n), fresh, id0)   # whole ciphertexts
    for level in (fresh + 1, -1):
        with pytest.raises(RuntimeError, match="level out of range"):
            V.import_half(halves[0], level, id0)
    for count in (0, K_ENC_MAX + 1):
        with pytest.raises(RuntimeError, match=rf"batch size outside 1\.\.{K_ENC_MAX}"):
            _raw_import(V, count, fresh)
    with pytest.raises(RuntimeError, match="id out of range"):
        V.import_half_many(halves, fresh, ((2 ** 40 - 2) << 16) | 5)   # the third member's counter would be 2^40
    with pytest.raises(RuntimeError, match="id out of range"):
        V.import_half(halves[0], fresh, 1 << 56)
    # one word EQUAL to its modulus: the error names member and row, nothing is stored
    nl = halves.shape[1]
    for member, row, col in ((0, 0, 0), (2, 1, 17), (1, nl - 1, n - 1)):
        bad = halves.copy()
        bad[member, row, col] = q[row]
        with pytest.raises(RuntimeError, match=rf"member {member}, row {row}\b.*nothing stored"):
            V.import_half_many(bad, fresh, id0)
    bad = halves[0].copy()
    bad[2, 5] = q[2]
    with pytest.raises(RuntimeError, match=r"member 0, row 2\b"):
        V.import_half(bad, fresh, id0)
    # --- both contexts still work, and hold no more than before
    gc.collect()                                             # handles the refusals' tracebacks still referred to
    covered_server(), covered_client()
    V.sync(), E.sync()
    assert V.pool_stats()["bytes"] <= before_v and E.pool_stats()["bytes"] <= before_e


# ---------------------------------------------------------------- 5. nothing else moved
def test_public_key_encryption_is_unmoved():
    """enc_ctr_ and the seeded counter are separate: public-key encryptions give the same words with seeded calls in
    between as without them; and a context without a mask key (a refused seeded call included) samples as ever.  That
    those residues are the oracle's stays with the untouched parity tests, whose engines have no mask key."""
    A, B = _engine("raw"), _engine("raw")
    z = _unit(A, 7, 3)
    want = [A.export(A.encrypt(v)) for v in z]
    B.encrypt_seeded(z[0])
    got = [B.export(B.encrypt(z[0]))]
    B.encrypt_seeded_many(z, level=1)
    got += [B.export(B.encrypt(v)) for v in z[1:]]
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    assert B.encrypt_seeded(z[0]).seed_id >> 16 == 4 and A.encrypt_seeded(z[0]).seed_id >> 16 == 0
    D0, D1 = _engine("raw", mask_key=None), _engine("raw", mask_key=None)
    with pytest.raises(RuntimeError, match="cannot be published"):
        D1.encrypt_seeded(z[0])
    assert np.array_equal(D0.export_pk(), D1.export_pk())
    assert all(np.array_equal(D0.export(D0.encrypt(v)), D1.export(D1.encrypt(v))) for v in z)
    assert not np.array_equal(D0.export_pk()[1], A.export_pk()[1])    # its a half is under the context key, as ever


# ---------------------------------------------------------------- 6. once, at the real shape
def test_the_real_shape_once(coeff_dir):
    """The 11 / 4 set at N = 2^16, FIPS true-FHE (the set of test_transcipher_end_to_end_with_no_secret_on_the_server):
    the client encrypts its AES key seeded, the pair crosses the wire as halves, the server -- built from the compressed
    bundle, no secret -- expands the key and transciphers one block, the client decodes the message bytes.  Then the
    22 round-key ciphertexts: seeded batched against 22 public-key encryptions, 22 half imports against 22 load_ct, a
    few passes each after one warm-up, host clock around calls that end in a stream synchronise.  Prints upload bytes
    and times; no time is asserted.  DESIGN.md §3.27 records one run."""
    from aes_keyschedule import expand_aes128_key, load_all_coeffs
    from ctr_mode import ctr_xor, fips_block_fn
    from engine_context import EngineContext
    from key_expansion import EncryptedRoundKeys
    from pipeline import AESPipeline
    from state_encoder import dump_ct, dump_ct_seeded, load_ct, load_ct_seeded
    co = load_all_coeffs(coeff_dir)
    client = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0x5EED, enc_nonce=0x5EED, mask_key=MASK)
    cpipe = AESPipeline(client, co, true_fhe=True, fips=True)
    rng = np.random.default_rng(0x5EED)
    master = rng.integers(0, 256, 16).astype(np.uint8)
    rks = expand_aes128_key(master)
    nonce = bytes(range(0x30, 0x3C))
    warm = ctr_xor(fips_block_fn(rks), rng.integers(0, 256, (1, 16)).astype(np.uint8), nonce, 3)
    cpipe.transcipher(warm, nonce, 3, cpipe.expand_key(*cpipe.encrypt_key(master)))   # the warm-up: every key now exists
    server = EngineContext.from_evaluation_keys(client.export_evaluation_keys(compressed=True, stream=True))
    assert server.secret_key is None and not server.engine.has_secret
    spipe = AESPipeline(server, co, true_fhe=True, fips=True)
    pair = cpipe.encrypt_key(master, seeded=True)
    wire = [dump_ct_seeded(client, c) for c in pair]
    seeded_bytes = sum(w[0].nbytes for w in wire)
    full_bytes = sum(dump_ct(client, c)[0].nbytes for c in pair)
    assert 2 * seeded_bytes == full_bytes
    skey = [load_ct_seeded(server, b, level, sid, tag) for b, level, tag, sid in wire]
    m = rng.integers(0, 256, (1, 16)).astype(np.uint8)
    counter0 = 2 ** 32 - 9
    c = ctr_xor(fips_block_fn(rks), m, nonce, counter0)
    out = [dump_ct(server, x) for x in spipe.transcipher(c, nonce, counter0, spipe.expand_key(*skey))]
    back = [load_ct(client, *w) for w in out]
    assert np.array_equal(cpipe.encoder.decode(*back).reshape(-1), m.reshape(-1))
    print(f"real shape (11 / 4, N = 2^16): key pair upload {seeded_bytes / 2 ** 20:.2f} MiB seeded, {full_bytes / 2 ** 20:.2f} MiB full")
    # --- the 22 round-key ciphertexts, both ways
    E, V = client.engine, server.engine
    enc = cpipe.encoder

    def seeded():
        pairs = enc.encode_many(rks, seeded=True)
        E.sync()
        return pairs

    def public():
        pairs = [enc.encode(k) for k in rks]
        E.sync()
        return pairs

    def timed(f, passes=5):
        f()
        ts = []
        for _ in range(passes):
            t = time.perf_counter()
            f()
            ts.append(1e3 * (time.perf_counter() - t))
        return min(ts), sorted(ts)[len(ts) // 2]

    t_seed, t_pub = timed(seeded), timed(public)
    erk = EncryptedRoundKeys.from_pairs(seeded(), cpipe.layout)
    recs = erk.dump_seeded(client)
    fulls = [dump_ct(client, x) for pr in erk.pairs for x in pr]
    assert 2 * sum(r[0].nbytes for r in recs) == sum(f[0].nbytes for f in fulls)

    def half_import():
        r = EncryptedRoundKeys.load_seeded(server, recs, spipe.layout)
        V.sync()
        return r

    def full_import():
        r = [load_ct(server, *f) for f in fulls]
        V.sync()
        return r

    t_half, t_full = timed(half_import), timed(full_import)
    serk = half_import()
    assert all(np.array_equal(V.export(x), f[0]) for x, f in zip([x for pr in serk.pairs for x in pr], fulls))
    print(f"22 round-key ciphertexts: encrypt {t_seed[0]:.2f} ms seeded batched (median {t_seed[1]:.2f}), {t_pub[0]:.2f} ms public-key "
          f"(median {t_pub[1]:.2f}); upload {sum(r[0].nbytes for r in recs) / 2 ** 20:.1f} MiB seeded, {sum(f[0].nbytes for f in fulls) / 2 ** 20:.1f} MiB full; "
          f"import {t_half[0]:.2f} ms as halves (median {t_half[1]:.2f}), {t_full[0]:.2f} ms full with check (median {t_full[1]:.2f})")
