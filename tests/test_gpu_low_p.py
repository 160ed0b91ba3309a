"""The per-level special basis (Engine.set_low_p / aesfhe_set_low_p).

A key switch at a level of nl < alpha limbs has one digit, so P only has to exceed Q_l by one prime: with the
option on it runs over the first nl + 1 special primes with that level's own single-digit keys.

Small set: N = 2^13, max_level 10, dnum 2 -> n_ks = 12, alpha = 6, n_p = 7.  Levels 0..3 (2..5 limbs) are
reduced, level 4 (6 limbs = alpha, one digit) is the first unreduced one, levels 5.. have two digits.

- off is the parent: an engine that had the option on and off again exports the same residues as one that never
  had it, for every key-switching entry point;
- on is correct: at every reduced level (and the boundary level) the decrypted results equal the plaintext
  computation, and the slot error with the option on stays within 2 x the largest error the SAME calls make with
  the option off over 8 seeds (the bound is measured from the off path in the test; nothing of the on path enters it).
  Measured on an MI355X, per (op, level), max over the 8 seeds: off-path error 1.7e-5 .. 5.0e-5, on-path error
  1.6e-5 .. 4.1e-5, on / off ratio 0.67 .. 1.37 (the test prints the table);
- row counts: one rotation at a reduced level tallies one key switch there (level_counters) and the NTT rows of
  nl + np(l) extended rows;
- a galois_multi batch with members at a reduced and an unreduced level has the separate calls' residues (asserted;
  each member is pinned against the oracle in tests/test_gpu_low_p_parity.py) and decrypts to the plaintext values;
- N = 2^16, the C2 7/4 set (EngineContext turns the option on): levels 1 and 7, one C2 encrypt (FIPS-197 bytes,
  precision margin no lower than the option-off margin of the same state by more than the recorded run-to-run
  range; measured 521x on, 509x off), one sparse bootstrap.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_N, LMAX, DNUM = 13, 10, 2
REDUCED = (0, 1, 2, 3)   # nl = 2..5 < alpha = 6
BOUNDARY = 4             # nl = alpha
SEEDS = 8


def _engine(seed=0x10F, low=None):
    from mi355x_ckks import Engine
    # defer_calls=False: every call runs when it is made (a separate call is then a separate key switch)
    E = Engine(log_n=LOG_N, max_level=LMAX, dnum=DNUM, seed=seed, allow_insecure=True, enc_nonce=seed, defer_calls=False)
    if low is not None:
        E.set_low_p(low)
    return E


@pytest.fixture(scope="module")
def E():
    e = _engine()
    assert (e.alpha, e.n_p) == (6, 7)
    return e


def _slots(E, rng):
    return np.exp(2j * np.pi * rng.random(E.slot_count))


def _ops(E, level, a, b, za, zb):
    """{name: (ciphertexts, expected slots)} of every key-switching entry point on a, b at `level`"""
    out = {}
    if level >= 1:
        # aesfhe_mul with relin = 1, settled at once so that the owed relinearisation + rescale run here and not
        # inside a later decrypt (which opens a deferred tensor with s^2): relin_rescale_tensor / relin_rescale;
        # and aesfhe_relinearize of the 3-polynomial tensor (relin_raw)
        r = E._raw_mul(a, b, True)
        E.settle(r)
        out["relin"] = ([r], [za * zb])
        out["relinearize"] = ([E.relinearize(E._raw_mul(a, b, False))], [za * zb])
        out["mul_many"] = (E.multiply_many([(a, b), (b, b), (a, a)]), [za * zb, zb * zb, za * za])
    out["conjugate"] = ([E.conjugate(a)], [np.conj(za)])
    out["rotate"] = ([E.rotate(a, delta=3)], [np.roll(za, 3)])
    for nb in (1, 2, 3):
        items = [(a, E.galois_rotate(1)), (b, E.galois_conj), (b, E.galois_rotate(-2))][:nb]
        want = [np.roll(za, 1), np.conj(zb), np.roll(zb, -2)][:nb]
        out[f"galois_multi{nb}"] = (E.galois_multi(items), want)
    st = E.rotate(E.stack([a, b]), delta=5)
    out["stacked_rotate"] = (E.unstack(st), [np.roll(za, 5), np.roll(zb, 5)])
    return out


def _inputs(E, level, seed):
    rng = np.random.default_rng(seed)
    za, zb = _slots(E, rng), _slots(E, rng)
    a, b = E.encrypt(za), E.encrypt(zb)
    if level < E.fresh_level:
        a, b = E.level_down(a, level), E.level_down(b, level)
    return a, b, za, zb


def _errors(E, level, seed):
    a, b, za, zb = _inputs(E, level, seed)
    return {k: max(float(np.abs(E.decrypt(c) - w).max()) for c, w in zip(cts, want))
            for k, (cts, want) in _ops(E, level, a, b, za, zb).items()}


def test_setting_and_basis_sizes(E):
    E.set_low_p(False)
    assert [E.ks_special_primes(l) for l in range(LMAX + 1)] == [7] * (LMAX + 1)
    E.set_low_p(True)
    try:
        assert [E.ks_special_primes(l) for l in REDUCED] == [E.nl(l) + 1 for l in REDUCED]
        assert [E.ks_special_primes(l) for l in range(BOUNDARY, LMAX + 1)] == [7] * (LMAX + 1 - BOUNDARY)
    finally:
        E.set_low_p(False)


def test_off_is_the_parent():
    """residues with the option off (after it had been on) == an engine that never had the option"""
    A, B = _engine(seed=0xA11), _engine(seed=0xA11)
    # A: the option on for a few key switches first (its reduced keys and tables then exist), then off
    A.set_low_p(True)
    a, b, za, zb = _inputs(A, 2, 1)
    A.decrypt(A.rotate(a, delta=1)), A.export(A._raw_mul(a, b, True))
    A.set_low_p(False)
    # the same number of encryptions on B: the encryption counter is part of the randomness
    _inputs(B, 2, 1)
    for level in (1, 3, BOUNDARY, 6):
        ia, ib = _inputs(A, level, 7), _inputs(B, level, 7)
        ra, rb = _ops(A, level, *ia), _ops(B, level, *ib)
        assert ra.keys() == rb.keys()
        for k in ra:
            for ca, cb in zip(ra[k][0], rb[k][0]):
                assert np.array_equal(A.export(ca), B.export(cb)), (level, k)
        assert all(c.num_polys == 2 for k in ("relin", "relinearize", "mul_many") for c in ra[k][0])


def test_on_is_correct_and_no_noisier(E):
    """every op at every reduced level (and the boundary level): on-path error <= 2 x max over 8 seeds of the
    off-path error of the same calls"""
    rows = []
    try:
        for level in REDUCED + (BOUNDARY,):
            E.set_low_p(False)
            off = [_errors(E, level, s) for s in range(SEEDS)]
            E.set_low_p(True)
            on = [_errors(E, level, s) for s in range(SEEDS)]
            for k in off[0]:
                off_max = max(e[k] for e in off)
                on_max = max(e[k] for e in on)
                rows.append((level, k, off_max, on_max))
    finally:
        E.set_low_p(False)
    for level, k, off_max, on_max in rows:
        print(f"low_p level {level} {k:15s} off max {off_max:.3e}  on max {on_max:.3e}  ratio {on_max / off_max:.2f}")
    for level, k, off_max, on_max in rows:
        assert off_max < 1e-3, (level, k, off_max)     # the plaintext computation itself (unit-modulus slots)
        assert on_max <= 2.0 * off_max, (level, k, off_max, on_max)


def test_row_counts(E):
    """one rotation at a reduced level is one key switch there (level_counters) over nl + np(l) extended rows"""
    def rotation(level):
        a, _, _, _ = _inputs(E, level, 3)
        E.rotate(a, delta=1)  # keys, tables
        E.reset_counters()
        E.rotate(a, delta=1)
        return E.counters()["ntt_rows"], E.level_counters()["key_switch"]
    try:
        for level in REDUCED:
            nl = E.nl(level)
            E.set_low_p(False)
            full, ks_full = rotation(level)
            E.set_low_p(True)
            low, ks_low = rotation(level)
            np_l = E.ks_special_primes(level)
            print(f"low_p rows level {level}: full {full}  low {low}")
            assert np_l == nl + 1 and ks_full == {level: 1} and ks_low == {level: 1}
            # NTT rows of the key switch: the INTT of d (nl), the forward NTT over the nl + np extended rows,
            # the ModDown INTT of both polynomials' P rows (2 np), its finish (2 nl)
            assert low == nl + (nl + np_l) + 2 * np_l + 2 * nl, (level, low)
            assert full == nl + (nl + E.n_p) + 2 * E.n_p + 2 * nl, (level, full)
    finally:
        E.set_low_p(False)


def test_mixed_level_batch(E):
    E.set_low_p(True)
    try:
        lo, _, zlo, _ = _inputs(E, 3, 11)        # reduced
        hi, _, zhi, _ = _inputs(E, 5, 12)        # two digits, full basis
        items = [(lo, E.galois_rotate(2)), (hi, E.galois_rotate(2)), (hi, E.galois_conj), (lo, E.galois_conj)]
        got = E.galois_multi(items)
        sep = [E.rotate(lo, delta=2), E.rotate(hi, delta=2), E.conjugate(hi), E.conjugate(lo)]
        want = [np.roll(zlo, 2), np.roll(zhi, 2), np.conj(zhi), np.conj(zlo)]
        for g, s, w in zip(got, sep, want):
            assert g.level == s.level
            # the batch is the separate calls, residue for residue (each member against the oracle:
            # tests/test_gpu_low_p_parity.py test_galois_multi_mixed_levels_bitexact)
            assert np.array_equal(E.export(g), E.export(s))
            dg, ds = E.decrypt(g), E.decrypt(s)
            # each side carries at most the key-switch error bounded above (2 x the off path's 5.0e-5)
            assert np.abs(dg - ds).max() < 2e-4
            assert np.abs(dg - w).max() < 1e-3
    finally:
        E.set_low_p(False)


# ---------------------------------------------------------------------------- N = 2^16, the C2 7/4 set
@pytest.fixture(scope="module")
def ctx9():
    from engine_context import EngineContext
    return EngineContext(signature=1, boot_fresh_level=7, dnum=4, thread_count=4, seed=0xC2C2, enc_nonce=0xC2C2)


def test_c2_set_levels_1_and_7(ctx9):
    E = ctx9.engine
    assert E.low_p and E.alpha == 10 and E.n_p == 11
    assert E.ks_special_primes(1) == 4 and E.ks_special_primes(7) == 10
    for level in (1, 7):
        try:
            E.set_low_p(False)
            off = [_errors(E, level, s) for s in range(SEEDS)]
            E.set_low_p(True)
            on = _errors(E, level, 0)
        finally:
            E.set_low_p(True)
        for k in on:
            off_max = max(e[k] for e in off)
            print(f"low_p C2 level {level} {k:15s} off max {off_max:.3e}  on {on[k]:.3e}")
            assert off_max < 1e-3 and on[k] <= 2.0 * off_max, (level, k, off_max, on[k])


def test_c2_encrypt_and_margin(ctx9):
    from aes_keyschedule import expand_aes128_key, load_all_coeffs
    from lut import ensure_coeffs
    from oracle import aes_plain
    from pipeline import AESPipeline
    assert ctx9.engine.low_p
    pipe = AESPipeline(ctx9, load_all_coeffs(ensure_coeffs()), use_hard_renorm_between_steps=True)
    rng = np.random.default_rng(99)
    rks = expand_aes128_key(rng.integers(0, 256, 16).astype(np.uint8))
    pt = rng.integers(0, 256, 16).astype(np.uint8)
    dbg = {}
    ct = pipe.encrypt(pt, rks, debug=dbg)
    assert np.array_equal(pipe.encoder.decode(*ct), aes_plain.ref_encrypt(pt, rks))
    assert dbg and all(v["plain"] is not None for v in dbg.values())
    # the bench's own precision measure (debug dict of one more encrypt), with the option on and off on the same
    # state: on may not fall below off by more than the full basis' recorded run-to-run range, 340-567x
    # (DESIGN.md §9), i.e. on >= off * 340 / 567
    from bench import measure_precision
    p = measure_precision(pipe, ctx9, rks, pt, "one C2 state")
    E = ctx9.engine
    try:
        E.set_low_p(False)
        p_off = measure_precision(pipe, ctx9, rks, pt, "one C2 state")
    finally:
        E.set_low_p(True)
    print(f"low_p C2 encrypt: margin factor on {p['margin_factor']:.0f} (worst stage {p['worst_stage']}), "
          f"off {p_off['margin_factor']:.0f} (worst stage {p_off['worst_stage']})")
    assert p["margin_factor"] >= p_off["margin_factor"] * 340.0 / 567.0


def test_c2_sparse_bootstrap(ctx9):
    from test_gpu_bootstrap import BOOT_TOL
    E = ctx9.engine
    assert E.low_p
    P = 32
    z = np.exp(2j * np.pi * np.random.default_rng(1).random(P))
    out = E.bootstrap_sparse(E.intt(ctx9.encrypt(np.tile(z, E.slot_count // P))), P)
    assert out.level == 7
    assert np.abs(ctx9.decrypt(out) - np.tile(z, E.slot_count // P)).max() < BOOT_TOL
