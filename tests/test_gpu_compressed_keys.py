"""Seed-compressed evaluation keys: a context built with a public MASK KEY draws the uniform `a` half
of every key under it, ships the `b` halves, and the server regenerates `a` on its device (k_complete_key).

Everything here is exact, word for word: the `a` halves against a numpy model of the PRF (tests/helpers/mask_prf.py),
the keys against the default context's through b + a s, the server's keys and results against the client's.  Sets:
RAW, LOWP and BOOT of tests/test_gpu_eval_context.py at N = 2^13, and once the 11 / 4 set at N = 2^16.
"""
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

pytestmark = pytest.mark.gpu

RAW = dict(log_n=13, max_level=6, dnum=3, allow_insecure=True)
LOWP = dict(log_n=13, max_level=10, dnum=2, allow_insecure=True)   # alpha = 6: levels 0..3 are reduced
BOOT = dict(log_n=13, use_bootstrap=True, max_level=3, dnum=5, allow_insecure=True)
SETS = {"raw": (RAW, False, 0xE7A1), "low_p": (LOWP, True, 0x10F), "boot": (BOOT, False, 7)}   # parameters, low-P, seed
MASK = bytes(range(0xA0, 0xC0))


def _context(which, mask_key=MASK):
    """an EngineContext over the set's engine (EngineContext's own constructor forms fix other levels)"""
    from engine_context import EngineContext
    params, low, seed = SETS[which]
    p = dict(params)
    if p.pop("use_bootstrap", False):
        C = EngineContext(signature=1, boot_fresh_level=p.pop("max_level"), seed=seed, enc_nonce=seed, mask_key=mask_key, **p)
    else:
        C = EngineContext(signature=2, seed=seed, enc_nonce=seed, mask_key=mask_key, **p)
    C.engine.set_low_p(low)
    return C


def _engine(which, mask_key=None, **over):
    from mi355x_ckks import Engine
    params, low, seed = SETS[which]
    E = Engine(**{**dict(seed=seed, enc_nonce=seed, mask_key=mask_key), **params, **over})
    E.set_low_p(low)
    return E


def _server_engine(which, mask_key=None):
    from mi355x_ckks import Engine
    params, low, _ = SETS[which]
    V = Engine.evaluation_only(enc_nonce=1, mask_key=mask_key, **params)
    V.set_low_p(low)
    return V


def _some_keys(E, which):
    """[(galois, level)]: key 0, one rotation key, and where the set has them the dense -> sparse key and one
    reduced-level key, each made resident"""
    ids = [(0, -1), (E.galois_rotate(1), -1)]
    if which == "boot":
        ids.append((2 * E.n + 1, -1))
    if which == "low_p":
        ids.append((E.galois_rotate(1), 2))
    for g, lv in ids:
        E.ensure_key(g, lv)
    return ids


def _key_view(E, g, level):
    """(key as [digits][2][nkey][N], prime index of each of the nkey rows, the a rows' stream id per digit)"""
    from mask_prf import stream_id
    flat = E.export_key(g, level)
    if level >= 0:
        nq_rows, digits, streams = E.nl(level), 1, [stream_id(10, g, level)]
    elif g == 2 * E.n + 1:
        nq_rows, digits, streams = 2, 1, [stream_id(4, g, 0)]
    else:
        nq_rows, digits, streams = E.n_ks, E.dnum, [stream_id(4, g, j) for j in range(E.dnum)]
    key = flat.reshape(digits, 2, -1, E.n)
    nkey = key.shape[2]
    primes = [l if l < nq_rows else E.n_q + (l - nq_rows) for l in range(nkey)]   # extmap(nq_rows): Q limbs, then P
    return key, primes, streams


@pytest.fixture(scope="module", params=list(SETS))
def client(request):
    """(set name, mask-key EngineContext with _some_keys resident)"""
    C = _context(request.param)
    assert C.engine.mask_key() == MASK
    return request.param, C, _some_keys(C.engine, request.param)


def test_a_halves_are_the_prf_under_the_mask_key(client):
    """every coefficient of every a row of pk, key 0, a rotation key, the dense -> sparse key (boot) and a reduced
    level's key (low_p) is prf(mask key, stream id, (prime << log_n) + k) mod q_prime: streams 2, 4 (per digit), 10"""
    from mask_prf import stream_id, uniform_rows
    which, C, ids = client
    E = C.engine
    q = E.moduli()
    pk = E.export_pk()
    assert np.array_equal(pk[1], uniform_rows(MASK, stream_id(2), range(E.n_q), q, E.log_n))
    for g, lv in ids:
        key, primes, streams = _key_view(E, g, lv)
        for j, st in enumerate(streams):
            assert np.array_equal(key[j, 1], uniform_rows(MASK, st, primes, q, E.log_n)), (g, lv, j)
            assert not np.array_equal(key[j, 0], key[j, 1])
    # and under no mask key the same rows come from the context key: another polynomial
    if which == "raw":
        D = _engine(which)
        assert D.mask_key() is None and not np.array_equal(D.export_pk()[1], pk[1])


def _mac(b, a, s, q):
    """b + a s mod q, rows against q[:, None]"""
    q = np.asarray(q, np.uint64).reshape(-1, 1)
    return (b.astype(np.uint64) + a.astype(np.uint64) * s.astype(np.uint64) % q) % q


def test_keys_are_the_default_keys_with_another_a(client):
    """b + a s (mod q_row) agrees word for word between the mask-key context and the default context of the same seed:
    e, s, s' and the gadget come from the context key's streams in both, only a differs.  The default context's keys
    are the ones tests/test_gpu_parity.py and tests/test_gpu_low_p_parity.py pin to the oracle.  The dense -> sparse
    key is taken under the sparse secret (export_sparse is its NTT form on every prime)."""
    which, C, ids = client
    M, D = C.engine, _engine(which)
    q = M.moduli().astype(np.uint64)
    s = M.export_secret()
    assert np.array_equal(s, D.export_secret())                 # the secret stays under the context key
    pm, pd = M.export_pk(), D.export_pk()
    assert not np.array_equal(pm[1], pd[1])
    assert np.array_equal(_mac(pm[0], pm[1], s[:M.n_q], q[:M.n_q]), _mac(pd[0], pd[1], s[:M.n_q], q[:M.n_q]))
    for g, lv in ids:
        D.ensure_key(g, lv)
        km, primes, _ = _key_view(M, g, lv)
        kd, _, _ = _key_view(D, g, lv)
        target = M.export_sparse() if g == 2 * M.n + 1 else s
        if g == 2 * M.n + 1:
            assert np.array_equal(target, D.export_sparse())
        for j in range(km.shape[0]):
            assert not np.array_equal(km[j, 1], kd[j, 1])
            assert np.array_equal(_mac(km[j, 0], km[j, 1], target[primes], q[primes]),
                                  _mac(kd[j, 0], kd[j, 1], target[primes], q[primes])), (g, lv, j)


def _inputs(E, seed, boot):
    rng = np.random.default_rng(seed)
    zs = [np.exp(2j * np.pi * rng.random(E.slot_count)) for _ in range(2)]
    if boot:
        per = lambda n: np.tile(0.5 * (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)), E.slot_count // n)
        zs += [per(16), per(E.slot_count)]
    cts = [E.encrypt(z) for z in zs]
    return [(E.export(c), c.level) for c in cts]


def _workload(E, wire, levels, boot):
    """one product with its relinearisation, two rotations, a conjugation and a galois_multi at each level; on the
    bootstrappable set one sparse and one full bootstrap"""
    cts = [E.import_ct(arr, lv) for arr, lv in wire]
    out = []
    for l in levels:
        a, b = E.level_down(cts[0], l), E.level_down(cts[1], l)
        r = E._raw_mul(a, b, True)
        E.settle(r)
        out += [r, E.rotate(a, delta=1), E.rotate(a, delta=5), E.conjugate(b)]
        out += E.galois_multi([(a, E.galois_rotate(2)), (a, E.galois_conj)])
    if boot:
        out += [E.bootstrap_sparse(cts[2], 16), E.bootstrap(cts[3])]
    return [E.export(c) for c in out]


def test_the_servers_keys_are_the_clients(client, tmp_path):
    from engine_context import EngineContext
    from evaluation_keys import CompressedEvaluationKeys, load_bundle
    which, C, _ = client
    E = C.engine
    boot = which == "boot"
    levels = {"raw": [3], "low_p": [6, 2], "boot": [2]}[which]
    wire = _inputs(E, 3, boot)
    want = _workload(E, wire, levels, boot)                       # the warm-up: its keys exist from here on
    ids = sorted(E.key_ids())
    assert any(lv >= 0 for _, lv in ids) == (which == "low_p")
    assert ((2 * E.n + 1, -1) in ids) == boot
    written = C.export_evaluation_keys(compressed=True, stream=True).save(tmp_path / "half")
    written_v1 = C.export_evaluation_keys(stream=True).save(tmp_path / "full")
    # exactly half: the 32-byte mask key lives in the header, not in the key files
    assert 2 * written == written_v1 == 4 * (2 * E.n_q * E.n + sum(E.ksk_words(g, lv) for g, lv in ids))
    bundle = load_bundle(tmp_path / "half")
    assert type(bundle) is CompressedEvaluationKeys and bundle.mask_key == MASK and bundle.nbytes() == written
    S = EngineContext.from_evaluation_keys(bundle, allow_insecure=True)
    V = S.engine
    assert not V.has_secret and S.secret_key is None and V.mask_key() == MASK
    assert sorted(V.key_ids()) == ids
    assert np.array_equal(V.export_pk(), E.export_pk())
    for g, lv in ids:
        assert np.array_equal(V.export_key(g, lv), E.export_key(g, lv)), (g, lv)
    got = _workload(V, wire, levels, boot)
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.shape == y.shape and np.array_equal(x, y), i
    # the uncompressed bundle of a mask-key context is an ordinary bundle: the same server, the same keys
    if which == "raw":
        S1 = EngineContext.from_evaluation_keys(load_bundle(tmp_path / "full"), allow_insecure=True)
        assert S1.engine.mask_key() is None
        assert all(np.array_equal(S1.engine.export_key(g, lv), E.export_key(g, lv)) for g, lv in ids)


def test_refusals_leave_the_context_usable():
    from engine_context import EngineContext
    key32, other = bytes(range(32)), bytes(range(1, 33))
    # --- setting the mask key
    K = _engine("raw", seed=key32)
    with pytest.raises(RuntimeError, match="equals the context key"):
        K.set_mask_key(key32)
    with pytest.raises(RuntimeError, match="equals the context key"):
        _engine("raw", seed=key32, mask_key=key32)
    assert K.mask_key() is None
    K.set_mask_key(other)                                        # still settable, and then set once
    with pytest.raises(RuntimeError, match="already set"):
        K.set_mask_key(MASK)
    assert K.mask_key() == other
    D = _engine("raw")                                           # no mask key
    pk = D.export_pk()                                           # key generation
    with pytest.raises(RuntimeError, match="keys already exist"):
        D.set_mask_key(MASK)
    assert D.mask_key() is None and np.array_equal(D.export_pk(), pk)
    # --- exports without a mask key
    for call in (D.export_pk_half, lambda: D.export_key_half(0, -1)):
        with pytest.raises(RuntimeError, match="cannot be compressed"):
            call()
    C = EngineContext(signature=2, seed=5, enc_nonce=5, **RAW)
    with pytest.raises(RuntimeError, match="cannot be compressed"):
        C.export_evaluation_keys(compressed=True)
    assert C.export_evaluation_keys().key_ids() == sorted(C.engine.key_ids())
    assert np.array_equal(D.export_key(0, -1), _engine("raw").export_key(0, -1))
    # --- imports
    M = _engine("raw", mask_key=MASK)
    half, pk_half = M.export_key_half(0, -1), M.export_pk_half()
    nkey, n, q = M.n_ks + M.n_p, M.n, [int(m) for m in M.moduli()]
    assert half.size == M.dnum * nkey * n == M.ksk_words(0, -1) // 2 and pk_half.shape == (M.n_q, n)
    assert np.array_equal(half.reshape(M.dnum, nkey, n), M.export_key(0, -1).reshape(M.dnum, 2, nkey, n)[:, 0])
    assert np.array_equal(pk_half, M.export_pk()[0])
    for E in (M, D):                                             # a keyed context takes no imports, mask key or not
        with pytest.raises(RuntimeError, match="secret key"):
            E.import_ksk_half(0, -1, half)
        with pytest.raises(RuntimeError, match="secret key"):
            E.import_pk_half(pk_half)
    U = _server_engine("raw")                                    # evaluation-only, no mask key
    with pytest.raises(RuntimeError, match="no mask key"):
        U.import_pk_half(pk_half)
    with pytest.raises(RuntimeError, match="no mask key"):
        U.import_ksk_half(0, -1, half)
    U.import_pk(M.export_pk())                                   # and it still takes whole keys
    U.import_ksk(0, -1, M.export_key(0, -1))
    V = _server_engine("raw", mask_key=MASK)
    with pytest.raises(RuntimeError, match="already set"):
        V.set_mask_key(other)
    with pytest.raises(RuntimeError, match="word count"):
        V.import_ksk_half(0, -1, half[:-1])
    with pytest.raises(RuntimeError, match="word count"):
        V.import_ksk_half(0, -1, M.export_key(0, -1))            # the whole key where its half belongs
    with pytest.raises(RuntimeError, match="word count"):
        V.import_pk_half(M.export_pk())
    with pytest.raises(RuntimeError, match="not a reduced level"):
        V.import_ksk_half(0, 0, half)                            # low-P off: no level is reduced
    # one residue EQUAL to its modulus in a middle row of the second digit; also the first P row (the LimbMap boundary)
    for digit, l, col in ((1, nkey // 2, 17), (1, M.n_ks, 0), (M.dnum - 1, nkey - 1, n - 1)):
        row = digit * nkey + l
        bad = half.copy()
        bad[row * n + col] = q[l if l < M.n_ks else M.n_q + l - M.n_ks]
        with pytest.raises(RuntimeError, match=rf"row {row}\b.*nothing stored"):
            V.import_ksk_half(0, -1, bad)
        assert V.key_ids() == []
    bad = pk_half.copy()
    bad[2, 5] = q[2]
    with pytest.raises(RuntimeError, match=r"row 2\b"):
        V.import_pk_half(bad)
    V.import_ksk_half(0, -1, half)                               # the correct import of the same key then succeeds
    V.import_pk_half(pk_half)
    assert V.key_ids() == [(0, -1)]
    assert np.array_equal(V.export_key(0, -1), M.export_key(0, -1)) and np.array_equal(V.export_pk(), M.export_pk())
    with pytest.raises(RuntimeError, match="already present"):
        V.import_ksk_half(0, -1, half)
    with pytest.raises(RuntimeError, match="already present"):
        V.import_pk_half(pk_half)
    with pytest.raises(RuntimeError, match="exports no halves"):
        V.export_key_half(0, -1)


def test_default_sampling_is_unchanged():
    """Without a mask key every draw is under the context key, as before: two contexts of one seed agree on pk and key
    0, and mask_key=None / False are that default.  That these residues are the ORACLE's stays with the existing,
    untouched parity tests (tests/test_gpu_parity.py, tests/test_gpu_low_p_parity.py), which build their engines
    without a mask key."""
    from engine_context import EngineContext
    A, B = _engine("raw"), _engine("raw", mask_key=None)
    C = EngineContext(signature=2, seed=SETS["raw"][2], enc_nonce=1, mask_key=False, **RAW)
    for E in (B, C.engine):
        assert E.mask_key() is None
        assert np.array_equal(E.export_pk(), A.export_pk()) and np.array_equal(E.export_key(0, -1), A.export_key(0, -1))
    R = EngineContext(signature=2, seed=SETS["raw"][2], enc_nonce=1, mask_key=True, **RAW)   # True: 32 fresh bytes
    assert len(R.engine.mask_key()) == 32 and not np.array_equal(R.engine.export_pk()[1], A.export_pk()[1])
    assert np.array_equal(R.engine.export_secret(), A.export_secret())


def test_the_real_shape_once():
    """The 11 / 4 set at N = 2^16: key 0, the conjugation key, the dense -> sparse key and one reduced-level key go
    through the compressed export and import and come out word for word; prints the wall time of the compressed
    import and of the uncompressed import of the same keys (one timed pass each, after the contexts exist).  No time
    is asserted; DESIGN.md §3.25 records one run."""
    from engine_context import EngineContext
    from evaluation_keys import CompressedEvaluationKeys, EvaluationKeys
    C = EngineContext(signature=1, boot_fresh_level=11, dnum=4, seed=0xC0DE, enc_nonce=0xC0DE, mask_key=MASK)
    E = C.engine
    assert E.low_p
    ids = [(0, -1), (E.galois_conj, -1), (2 * E.n + 1, -1), (E.galois_rotate(1), 0)]
    for g, lv in ids:
        E.ensure_key(g, lv)
    assert sorted(E.key_ids()) == sorted(ids)
    half, full = C.export_evaluation_keys(compressed=True), C.export_evaluation_keys()
    assert isinstance(half, CompressedEvaluationKeys) and isinstance(full, EvaluationKeys)
    assert 2 * half.nbytes() == full.nbytes()
    params = dict(log_n=E.log_n, max_level=E.fresh_level, dnum=E.dnum, use_bootstrap=True)
    # untimed: each path's first launch on engines of their own, and one small transform on each server's stream (a new
    # engine's first submission cost 8-20 ms in the runs behind DESIGN.md §3.25, whichever import came first)
    _eval_engine(params, MASK).import_pk_half(half.pk)
    _eval_engine(params, None).import_pk(full.pk)
    V, W = _eval_engine(params, MASK), _eval_engine(params, None)
    rows = np.ones((1, E.n), np.uint32)
    V.debug_ntt(rows, 0), W.debug_ntt(rows, 0)
    V.sync(), W.sync()
    t0 = time.perf_counter()
    V.import_pk_half(half.pk)
    for (g, lv), arr in half.items():
        V.import_ksk_half(g, lv, arr)
    V.sync()
    t1 = time.perf_counter()
    W.import_pk(full.pk)
    for (g, lv), arr in full.items():
        W.import_ksk(g, lv, arr)
    W.sync()
    t2 = time.perf_counter()
    for g, lv in ids:
        want = E.export_key(g, lv)
        assert np.array_equal(V.export_key(g, lv), want) and np.array_equal(W.export_key(g, lv), want), (g, lv)
    assert np.array_equal(V.export_pk(), E.export_pk())
    print(f"real shape (11 / 4, N = 2^16, pk + {len(ids)} keys): bundle {full.nbytes() / 2 ** 20:.1f} MiB full, "
          f"{half.nbytes() / 2 ** 20:.1f} MiB compressed; import {1e3 * (t2 - t1):.1f} ms full, {1e3 * (t1 - t0):.1f} ms compressed "
          f"(compressed / full = {(t1 - t0) / (t2 - t1):.2f})")


def _eval_engine(params, mask_key):
    from mi355x_ckks import Engine
    V = Engine.evaluation_only(enc_nonce=1, mask_key=mask_key, **params)
    V.set_low_p(True)
    return V
