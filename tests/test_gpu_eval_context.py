"""The evaluation-only context: a server that holds the public key and the switching keys it was
given, and never the secret.

Bit-exactness is the yardstick throughout: switching keys and ciphertexts travel as they are, encryption randomness
plays no part in an evaluation, so every output of the evaluation-only engine equals the keyed engine's word for
word.  Sets: the N = 2^13 raw sets of tests/test_gpu_parity.py (6 / 3) and tests/test_gpu_low_p.py (10 / 2, reduced
levels), the bootstrappable 2^13 set of tests/test_gpu_sparse_boot.py, and the 11 / 4 true-FHE set of
tests/test_gpu_true_fhe.py for the end-to-end transciphering.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAW = dict(log_n=13, max_level=6, dnum=3, allow_insecure=True)
LOWP = dict(log_n=13, max_level=10, dnum=2, allow_insecure=True)   # alpha = 6: levels 0..3 are reduced
BOOT = dict(log_n=13, use_bootstrap=True, max_level=3, dnum=5, allow_insecure=True)
ENC_TOL = 2e-4  # tests/test_gpu_parity.py::test_encrypt_decrypt_cross: fresh-encryption noise of a round trip


def _keyed(params, seed, low=False, enc_nonce=None):
    from mi355x_ckks import Engine
    E = Engine(seed=seed, enc_nonce=seed if enc_nonce is None else enc_nonce, **params)
    E.set_low_p(low)
    return E


def _server(K, params, keys=None, pk=True):
    """an evaluation-only engine of K's parameter set holding K's public key and `keys` (None: all present)"""
    from mi355x_ckks import Engine
    V = Engine.evaluation_only(enc_nonce=1, **params)
    assert np.array_equal(V.moduli(), K.moduli())
    V.set_low_p(K.low_p)
    if pk:
        V.import_pk(K.export_pk())
    for g, lv in (K.key_ids() if keys is None else keys):
        V.import_ksk(g, lv, K.export_key(g, lv))
    return V


def _inputs(E, seed):
    rng = np.random.default_rng(seed)
    za, zb = (np.exp(2j * np.pi * rng.random(E.slot_count)) for _ in range(2))
    a, b = E.encrypt(za), E.encrypt(zb)
    return [(E.export(a), a.level), (E.export(b), b.level)]


def _workload(E, wire, levels):
    """every key-switching entry point of the issue's list on the two imported inputs, at each of `levels`"""
    a0, b0 = (E.import_ct(arr, lv) for arr, lv in wire)
    out = []
    for l in levels:
        a, b = E.level_down(a0, l), E.level_down(b0, l)
        r = E._raw_mul(a, b, True)
        E.settle(r)                                   # ct x ct, relinearisation fused with the rescale
        out.append(r)
        out += [E.rotate(a, delta=1), E.rotate(a, delta=5), E.conjugate(b)]
        out += E.galois_multi([(a, E.galois_rotate(2)), (a, E.galois_conj)])   # two elements on one source
        out += E.rotate_many(a, [3, 7])               # hoisted
        out.append(E.conjugate(E._raw_mul(a, b, True)))   # a deferred 3-polynomial tensor: the tag_sq key
    return [E.export(c) for c in out]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), i


@pytest.fixture(scope="module")
def raw():
    """(keyed engine, inputs, its outputs) on the 6 / 3 set, low-P off"""
    K = _keyed(RAW, 0xE7A1)
    wire = _inputs(K, 1)
    return K, wire, _workload(K, wire, [3])


@pytest.mark.parametrize("which", ["raw", "low_p"])
def test_bit_exact_evaluation(raw, which):
    if which == "raw":
        K, wire, want = raw
        params, levels = RAW, [3]
    else:
        K, params, levels = _keyed(LOWP, 0x10F, low=True), LOWP, [6, 2]
        assert (K.alpha, K.n_p) == (6, 7)
        wire = _inputs(K, 2)
        want = _workload(K, wire, levels)
    ids = K.key_ids()
    n2 = 2 * K.n
    assert any(2 * n2 < g < 3 * n2 for g, _ in ids), "the workload made no tag_sq key"
    assert any(lv >= 0 for _, lv in ids) == (which == "low_p"), ids   # reduced-level keys travel on the low-P set only
    assert K.has_secret
    V = _server(K, params)
    assert not V.has_secret and sorted(V.key_ids()) == sorted(ids)
    _same(_workload(V, wire, levels), want)


def test_bootstrap_bit_exact():
    K = _keyed(BOOT, 7, enc_nonce=0)  # the set of tests/test_gpu_sparse_boot.py
    rng = np.random.default_rng(16)
    per = lambda n: np.tile(0.5 * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)), K.slot_count // n)
    cts = [K.encrypt(per(16)), K.encrypt(per(16)), K.encrypt(per(K.slot_count))]
    wire = [(K.export(c), c.level) for c in cts]

    def run(E):
        x, y, z = (E.import_ct(arr, lv) for arr, lv in wire)
        out = [E.bootstrap_sparse(x, 16)]
        out += list(E.bootstrap_pair_sparse(x, y, 16))
        out.append(E.bootstrap(z))
        return [E.export(c) for c in out]

    want = run(K)
    ids = K.key_ids()
    n2 = 2 * K.n
    assert (n2 + 1, -1) in ids and (n2 + 3, -1) in ids               # dense -> sparse, sparse -> dense
    assert any(4 * n2 < g < 5 * n2 for g, _ in ids)                   # the rotated sparse -> dense tags
    V = _server(K, BOOT)
    _same(run(V), want)


def test_missing_key_is_an_error_and_leaves_the_context_usable(raw):
    K, wire, _ = raw
    g9 = K.galois_rotate(9)
    V = _server(K, RAW)
    assert (g9, -1) not in V.key_ids()

    def covered(E):
        a, b = (E.import_ct(arr, lv) for arr, lv in wire)
        x = E._raw_mul(E.level_down(a, 3), E.level_down(b, 3), True)   # owes its rescale: the rotation normalises a copy
        return x, E.export(E.rotate(x, delta=1))

    _, want = covered(K)
    x, got = covered(V)
    assert np.array_equal(got, want)
    V.sync()
    before = V.pool_stats()["bytes"]
    for call in (lambda: V.rotate(x, delta=9), lambda: V.rotate_many(x, [1, 9]),
                 lambda: V.galois_multi([(x, K.galois_rotate(1)), (x, g9)])):
        with pytest.raises(RuntimeError, match="evaluation key missing") as ei:
            r = call()
            V.export(r[0] if isinstance(r, list) else r)
        assert str(g9) in str(ei.value) and "level -1" in str(ei.value)
    assert np.array_equal(V.export(V.rotate(x, delta=1)), want)   # the next, covered, operation: bit-exact
    V.sync()
    # a buffer the failed calls had kept would have made the repeat above allocate a new one
    assert V.pool_stats()["bytes"] == before


def _client_ctx_13(seed=0xC13):
    from engine_context import EngineContext
    return EngineContext(signature=2, max_level=6, log_n=13, seed=seed, enc_nonce=seed, allow_insecure=True)


def test_secret_is_refused(raw):
    from engine_context import EngineContext
    K, wire, _ = raw
    assert K._lib.aesfhe_has_secret(K._ctx.ptr) == 1
    C = _client_ctx_13()
    rng = np.random.default_rng(4)
    z = np.exp(2j * np.pi * rng.integers(0, 16, C.engine.slot_count) / 16)
    c = C.encrypt(z)
    C.engine.export(C.rotate(c, 1))
    S = EngineContext.from_evaluation_keys(C.export_evaluation_keys(), allow_insecure=True)
    V = S.engine
    assert V._lib.aesfhe_has_secret(V._ctx.ptr) == 0 and S.secret_key is None and S.evaluation_only
    hi, lo = (V.import_ct(C.engine.export(c), c.level) for _ in range(2))
    calls = {
        "decrypt": lambda: S.decrypt(hi),
        "renorm_pair": lambda: S.renorm_pair(hi, lo),
        "renorm_single": lambda: S.renorm_single(hi),
        "renorm_periodic": lambda: S.renorm_periodic(hi, lo, 16),
        "renorm_unpack": lambda: S.renorm_unpack(hi, 16),
        "renorm_pack": lambda: S.renorm_pack(hi, lo, 16),
        "export_secret": V.export_secret,
        "export_sparse": lambda: V._ctx.check(V._lib.aesfhe_export_sparse(V._ctx.ptr, np.zeros(1, np.uint32))),
        "create_secret_key": V.create_secret_key,
        "keygen": lambda: V._ctx.check(V._lib.aesfhe_keygen(V._ctx.ptr)),
    }
    for name, f in calls.items():
        with pytest.raises(RuntimeError, match="no secret key"):
            f()
    # still usable, and still the client's arithmetic
    assert np.array_equal(V.export(S.rotate(hi, 1)), C.engine.export(C.rotate(c, 1)))


def test_import_refusals(raw):
    K, wire, _ = raw
    V = _server(K, RAW, keys=[])
    key = K.export_key(0, -1)
    nkey, n, q = K.n_ks + K.n_p, K.n, [int(m) for m in K.moduli()]
    rows = K.dnum * 2 * nkey
    assert key.size == rows * n and V.ksk_words(0, -1) == key.size
    # a residue EQUAL to its row's modulus: word 0 of row 0, the last word of the last P row, the first word of the
    # first P row (the LimbMap boundary: row n_ks is special prime 0, not Q limb n_ks)
    for row, col, prime in ((0, 0, 0), (rows - 1, n - 1, K.n_q + K.n_p - 1), (K.n_ks, 0, K.n_q)):
        bad = key.copy()
        bad[row * n + col] = q[prime]
        assert q[prime] < 2 ** 32
        with pytest.raises(RuntimeError, match=rf"row {row}\b"):
            V.import_ksk(0, -1, bad)
        assert V.key_ids() == []                      # nothing stored
    # the last Q row holds residues below ITS prime only: one below the first special prime is refused there
    if q[K.n_ks - 1] < q[K.n_q]:
        bad = key.copy()
        bad[(K.n_ks - 1) * n] = q[K.n_ks - 1]
        with pytest.raises(RuntimeError, match=rf"row {K.n_ks - 1}\b"):
            V.import_ksk(0, -1, bad)
    with pytest.raises(RuntimeError, match="word count"):
        V.import_ksk(0, -1, key[:-1])
    with pytest.raises(RuntimeError, match="not a reduced level"):
        V.import_ksk(0, 0, key)                       # low-P off: no level is reduced
    V.import_ksk(0, -1, key)                          # the unmodified key is accepted
    assert V.key_ids() == [(0, -1)]
    with pytest.raises(RuntimeError, match="already present"):
        V.import_ksk(0, -1, key)
    with pytest.raises(RuntimeError, match="already present"):
        V.import_pk(K.export_pk())
    with pytest.raises(RuntimeError, match="secret key"):
        K.import_ksk(K.galois_rotate(3), -1, key)     # a keyed context takes no imports
    with pytest.raises(RuntimeError, match="secret key"):
        K.import_pk(K.export_pk())
    # another parameter set: max_level 5 into 6
    K5 = _keyed(dict(RAW, max_level=5), 0xE7A1)
    K5.encrypt(np.ones(4))
    with pytest.raises(RuntimeError, match="word count"):
        V.import_ksk(K5.galois_conj, -1, K5.export_key(K5.galois_conj, -1))
    with pytest.raises(RuntimeError, match="word count"):
        _server(K, RAW, keys=[], pk=False).import_pk(K5.export_pk())
    # Engine.check: the same pass over a ciphertext handle
    arr, lv = wire[0]
    assert V.check(V.import_ct(arr, lv)) is None
    nl = arr.shape[1]
    for poly, limb in ((0, 0), (1, 2), (1, nl - 1)):
        bad = arr.copy()
        bad[poly, limb, n - 1] = q[limb]
        assert V.check(V.import_ct(bad, lv)) == poly * nl + limb


def test_bundle_of_another_parameter_set_is_refused():
    from engine_context import EngineContext
    from evaluation_keys import EvaluationKeys
    C5 = EngineContext(signature=2, max_level=5, log_n=13, seed=5, enc_nonce=5, allow_insecure=True)
    b = C5.export_evaluation_keys()
    h = dict(b.header, max_level=6)   # its moduli are the 5-level chain's
    with pytest.raises(ValueError, match="moduli"):
        EngineContext.from_evaluation_keys(EvaluationKeys(h, b.pk, {k: b[k] for k in b.key_ids()}), allow_insecure=True)


def test_server_side_encryption_decrypts_on_the_client(raw):
    K, _, _ = raw
    V = _server(K, RAW, keys=[])
    rng = np.random.default_rng(6)
    z = np.exp(2j * np.pi * rng.random(K.slot_count))
    c = V.encrypt(z)
    back = K.import_ct(V.export(c), c.level)
    err = np.abs(K.decrypt(back) - z).max()
    print(f"server-side encryption: max slot error {err:.3g}")
    assert err < ENC_TOL
    # the server's samples are its own: another prng_key, another ciphertext of the same message
    V2 = _server(K, RAW, keys=[])
    assert not np.array_equal(V2.export(V2.encrypt(z)), V.export(c))


def test_disk_round_trip(raw, tmp_path):
    from engine_context import EngineContext
    from evaluation_keys import EvaluationKeys
    K, wire, want = raw
    C = EngineContext(signature=2, log_n=13, max_level=6, dnum=3, seed=0xE7A1, enc_nonce=0xE7A1, allow_insecure=True)
    _same(_workload(C.engine, wire, [3]), want)       # the same client: the same seed, the same keys
    written = C.export_evaluation_keys(stream=True).save(tmp_path / "keys")
    assert written == 4 * (2 * C.engine.n_q * C.engine.n + sum(C.engine.ksk_words(g, lv) for g, lv in C.engine.key_ids()))
    S = EngineContext.from_evaluation_keys(EvaluationKeys.load(tmp_path / "keys"), allow_insecure=True)
    assert S.secret_key is None and sorted(S.engine.key_ids()) == sorted(C.engine.key_ids())
    _same(_workload(S.engine, wire, [3]), want)


def test_transcipher_end_to_end_with_no_secret_on_the_server(coeff_dir):
    """the set of test_true_fhe_c2_on_the_bench_set: the client warms up, exports (streamed), the server transciphers
    another block under the imported keys and the client decodes FIPS-197 CTR bytes.

    One-off wall times of this test on an MI355X are recorded in DESIGN.md §3.24."""
    from aes_keyschedule import expand_aes128_key, load_all_coeffs
    from ctr_mode import ctr_xor, fips_block_fn
    from engine_context import EngineContext
    from key_expansion import EncryptedRoundKeys
    from pipeline import AESPipeline
    from state_encoder import dump_ct, load_ct
    t0 = time.perf_counter()
    co = load_all_coeffs(coeff_dir)
    client = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xE2E, enc_nonce=0xE2E)
    cpipe = AESPipeline(client, co, true_fhe=True, fips=True)
    rng = np.random.default_rng(0xE2E)
    rks = expand_aes128_key(rng.integers(0, 256, 16).astype(np.uint8))
    erk = EncryptedRoundKeys.from_pairs([cpipe.encoder.encode(k) for k in rks], cpipe.layout)
    nonce = bytes(range(0x30, 0x3C))
    warm = ctr_xor(fips_block_fn(rks), rng.integers(0, 256, (1, 16)).astype(np.uint8), nonce, 3)
    cpipe.transcipher(warm, nonce, 3, erk)            # the warm-up: every key the workload touches now exists
    t1 = time.perf_counter()
    server = EngineContext.from_evaluation_keys(client.export_evaluation_keys(stream=True))
    t2 = time.perf_counter()
    assert server.secret_key is None and not server.engine.has_secret
    with pytest.raises(ValueError, match="secret key"):
        AESPipeline(server, co, use_hard_renorm_between_steps=True)
    spipe = AESPipeline(server, co, true_fhe=True, fips=True)
    wire = [[dump_ct(client, c) for c in pr] for pr in erk.pairs]
    serk = EncryptedRoundKeys.from_pairs([tuple(load_ct(server, *w) for w in pr) for pr in wire], spipe.layout)
    m = rng.integers(0, 256, (1, 16)).astype(np.uint8)
    counter0 = 2 ** 32 - 9
    c = ctr_xor(fips_block_fn(rks), m, nonce, counter0)   # a different block, a different counter
    out = [dump_ct(server, x) for x in spipe.transcipher(c, nonce, counter0, serk)]
    t3 = time.perf_counter()
    back = [load_ct(client, *w) for w in out]
    assert np.array_equal(cpipe.encoder.decode(*back).reshape(-1), m.reshape(-1))
    nkeys = len(server.engine.key_ids())
    nbytes = 4 * sum(server.engine.ksk_words(g, lv) for g, lv in server.engine.key_ids())
    print(f"e2e: client set-up + warm-up {t1 - t0:.1f} s, export + import of {nkeys} keys ({nbytes / 2 ** 30:.2f} GiB) "
          f"{t2 - t1:.1f} s, server transcipher {t3 - t2:.1f} s, total {time.perf_counter() - t0:.1f} s")
