"""Residue-for-residue parity of the reduced-basis (low-P) key switch with the CPU oracle.

With Engine.set_low_p on, a key switch at a level of nl < alpha limbs runs over Q_l P_l, P_l = the first nl + 1 special
primes, with its own tables (engine.hip build_low_basis), its own single-digit keys (ksk_at, PRNG streams 10 / 11) and
its own ModDown-fused-with-rescale table.  tests/test_gpu_low_p.py bounds its slot error; here every entry point is
pinned against oracle/ckks_oracle.c (orc_gen_ksk_low / orc_keyswitch_low, themselves checked on the CPU by
tests/test_oracle_low_p.py).  Inputs are uniform random residues (every limb's full range), every assertion is
np.array_equal on exported residues, and Engine.export_ksk_at tells a key mismatch from a kernel mismatch.

Small set: N = 2^13, max_level 10, dnum 2 -> alpha 6, n_p 7; levels 0..3 reduced, level 4 (nl = alpha) the first
unreduced one, levels 5.. two digits.
Unfused-ModDown fallback: N = 2^13, max_level 14, dnum 1 -> alpha 16, n_p 17; at level 13 (nl = 15, np = 16) the
fused ModDown + rescale would need 1 + 16 > 16 conversion sources, so build_low_basis leaves it out and the
relinearisation runs its ModDown and the rescale separately; level 12 (nl = 14, 1 + 15 sources) still fuses.
C2 set: N = 2^16, EngineContext(signature=1, boot_fresh_level=7, dnum=4) -> alpha 10, n_p 11, the option on by default.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_N, LMAX, DNUM, SEED = 13, 10, 2, 0x10F
REDUCED = (0, 1, 2, 3)
UNREDUCED = (4, 6)       # nl = alpha (one digit, full basis); two digits


def rand_rows(O, nl, rng):
    return np.stack([rng.integers(0, int(O.moduli[t]), O.n, dtype=np.uint64) for t in range(nl)]).astype(np.uint32)


def rand_ct(O, level, npoly, rng):
    return np.stack([rand_rows(O, O.nl(level), rng) for _ in range(npoly)])


def addmod(a, b, q):
    return ((a.astype(np.uint64) + b) % q).astype(np.uint32)


class Ref:
    """the oracle's side of one parameter set: keys made once, and the compositions the engine's entry points are"""

    def __init__(self, O):
        self.O = O
        self._low, self._full = {}, {}

    def reduced(self, level):
        return self.O.nl(level) < self.O.alpha

    def low_key(self, g, level):
        if (g, level) not in self._low:
            self._low[g, level] = self.O.gen_ksk_low(g, level)
        return self._low[g, level]

    def full_key(self, g):
        if g not in self._full:
            self._full[g] = self.O.gen_ksk(g)
        return self._full[g]

    def keyswitch(self, level, g, d):
        if self.reduced(level):
            return self.O.keyswitch_low(level, [d], [self.low_key(g, level)])
        return self.O.keyswitch(level, d, self.full_key(g))

    def relin(self, level, t):
        """(d0, d1) + KS(d2) of a 3-polynomial tensor"""
        return addmod(t[:2], self.keyswitch(level, 0, t[2]), self.O.limbs_mod(self.O.nl(level)))

    def mul_relin_rescale(self, level, x, y):
        """tensor, relinearise, rescale.  The engine fuses the last two on the levels that have the table (one ModDown by
        P_l * q_l); with centred conversions (X - [X]_{PD}) / PD == (Y - [Y]_D) / D for X = P Y + [X]_P, so this two-step
        composition is matched bit for bit (as tests/test_gpu_parity.py has it for the full basis)"""
        return self.O.rescale(level, self.relin(level, self.O.tensor(level, x, y)))

    def galois(self, level, g, x):
        """automorphism, key switch of the second polynomial, the first added"""
        ax = self.O.automorph(level, g, x)
        ks = self.keyswitch(level, g, ax[1])
        ks[0] = addmod(ks[0], ax[0], self.O.limbs_mod(self.O.nl(level)))
        return ks


def _pair(max_level, dnum, seed):
    from mi355x_ckks import Engine
    from oracle.ckks_cpu import OracleParams
    # as tests/test_gpu_low_p.py: defer_calls=False, every call runs when it is made
    E = Engine(log_n=LOG_N, max_level=max_level, dnum=dnum, seed=seed, allow_insecure=True, enc_nonce=seed, defer_calls=False)
    E.set_low_p(True)
    O = OracleParams(log_n=LOG_N, max_level=max_level, dnum=dnum, seed=seed)
    assert np.array_equal(E.moduli(), O.moduli)
    assert (E.alpha, E.n_p, E.n_ks) == (O.alpha, O.n_p, O.n_ks)
    return E, Ref(O)


@pytest.fixture(scope="module")
def small():
    E, R = _pair(LMAX, DNUM, SEED)
    assert (E.alpha, E.n_p) == (6, 7)
    assert [E.ks_special_primes(l) for l in REDUCED + UNREDUCED] == [3, 4, 5, 6, 7, 7]
    return E, R


def _tags(E):
    return {"relin": 0, "conj": E.galois_conj, "rot": E.galois_rotate(-(E.slot_count // 4)), "conj_sq": 4 * E.n + E.galois_conj}


# ---------------------------------------------------------------------------- 1. keys
@pytest.mark.parametrize("which", ["relin", "conj", "rot", "conj_sq"])
def test_reduced_keys_bitexact(small, which):
    E, R = small
    g = _tags(E)[which]
    for level in REDUCED:
        key = E.export_ksk_at(g, level)
        assert key.shape == (2, 2 * E.nl(level) + 1, E.n)
        assert np.array_equal(key, R.low_key(g, level)), (which, level)
    for level in UNREDUCED:  # the full key serves from nl = alpha on
        assert np.array_equal(E.export_ksk_at(g, level), R.full_key(g)), (which, level)


# ---------------------------------------------------------------------------- 2. the raw switch
@pytest.mark.parametrize("which", ["relin", "conj", "rot"])
def test_keyswitch_bitexact(small, which):
    E, R = small
    g = _tags(E)[which]
    rng = np.random.default_rng(2)
    for level in REDUCED:
        d = rand_rows(R.O, E.nl(level), rng)
        assert np.array_equal(E.debug_keyswitch(level, g, d), R.O.keyswitch_low(level, [d], [R.low_key(g, level)])), (which, level)
    for level in UNREDUCED:  # the option still on: the selection picks the full basis and the full key
        d = rand_rows(R.O, E.nl(level), rng)
        assert np.array_equal(E.debug_keyswitch(level, g, d), R.O.keyswitch(level, d, R.full_key(g))), (which, level)


# ---------------------------------------------------------------------------- 3. fused relinearise + rescale
def _check_mul(E, R, level, rng):
    """E.multiply(x, y, "rlk") on both of its routes: eager (relinearised and rescaled straight from the factors,
    relin_rescale_tensor) and lazy (a deferred tensor, resolved by the export: relin_rescale)"""
    x, y = rand_ct(R.O, level, 2, rng), rand_ct(R.O, level, 2, rng)
    want = R.mul_relin_rescale(level, x, y)
    was = E.lazy
    try:
        for lazy in (False, True):
            E.set_lazy(lazy)
            got = E._raw_mul(E.import_ct(x, level), E.import_ct(y, level), True)
            assert got.level == level - 1 and got.num_polys == 2  # owed work is invisible
            assert np.array_equal(E.export(got), want), (level, "lazy" if lazy else "eager")
    finally:
        E.set_lazy(was)


def test_multiply_relin_rescale_bitexact(small):
    E, R = small
    rng = np.random.default_rng(3)
    for level in (1, 2, 3):
        _check_mul(E, R, level, rng)


# ---------------------------------------------------------------------------- 4. relinearize, no rescale
def test_relinearize_bitexact(small):
    E, R = small
    rng = np.random.default_rng(4)
    for level in REDUCED:
        t = R.O.tensor(level, rand_ct(R.O, level, 2, rng), rand_ct(R.O, level, 2, rng))
        got = E.relinearize(E.import_ct(t, level))  # an imported tensor owes no rescale
        assert got.level == level and got.num_polys == 2
        assert np.array_equal(E.export(got), R.relin(level, t)), level
    for level in (1, 2, 3):
        # the engine's own tensor owes its rescale: relinearize settles it too, the two steps run separately here
        x, y = rand_ct(R.O, level, 2, rng), rand_ct(R.O, level, 2, rng)
        t = E._raw_mul(E.import_ct(x, level), E.import_ct(y, level), False)
        assert np.array_equal(E.export(t), R.O.tensor(level, x, y))
        assert np.array_equal(E.export(E.relinearize(t)), R.mul_relin_rescale(level, x, y)), level


# ---------------------------------------------------------------------------- 5. rotate, conjugate
def test_rotate_conjugate_bitexact(small):
    E, R = small
    rng = np.random.default_rng(5)
    for level in (0, 3):
        x = rand_ct(R.O, level, 2, rng)
        cx = E.import_ct(x, level)
        for steps in (1, -(E.slot_count // 4)):
            assert np.array_equal(E.export(E.rotate(cx, delta=steps)), R.galois(level, E.galois_rotate(steps), x)), (level, steps)
        assert np.array_equal(E.export(E.conjugate(cx)), R.galois(level, E.galois_conj, x)), level


# ---------------------------------------------------------------------------- 6. conjugation of a deferred tensor
def test_conjugate_of_deferred_tensor_bitexact(small):
    """conjugate() of a lazy product (3 polynomials owing a rescale; engine.hip galois_lazy): sigma(c1) and sigma(c2) are
    switched with the keys sigma(s) -> s and sigma(s)^2 -> s, summed in Q_l P_l before the ONE ModDown, sigma(c0) added;
    the rescale stays owed and the export settles it.  The conjugation reads its sources reversed instead of permuting
    them; the export is in NTT form either way (export_ct brings a ciphertext there), so no E.ntt is needed"""
    E, R = small
    O = R.O
    g = E.galois_conj
    rng = np.random.default_rng(6)
    for level in (1, 3):
        x, y = rand_ct(O, level, 2, rng), rand_ct(O, level, 2, rng)
        t = E._raw_mul(E.import_ct(x, level), E.import_ct(y, level), True)
        E.reset_counters()
        got = E.conjugate(t)
        # two key switches, no relinearisation and no rescale: the tensor went through unresolved
        cnt = E.counters()
        assert (cnt["keyswitch"], cnt["relin"], cnt["rescale"]) == (2, 0, 0)
        ax = O.automorph(level, g, O.tensor(level, x, y))
        ks = O.keyswitch_low(level, [ax[1], ax[2]], [R.low_key(g, level), R.low_key(4 * E.n + g, level)])
        ks[0] = addmod(ks[0], ax[0], O.limbs_mod(O.nl(level)))
        assert got.level == level - 1
        assert np.array_equal(E.export(got), O.rescale(level, ks)), level


# ---------------------------------------------------------------------------- 7. batched entry points
@pytest.mark.parametrize("pairs", [3, 11])
def test_multiply_many_bitexact(small, pairs):
    """each member of one aesfhe_mul_many call against the oracle's single product; 11 pairs are more than one
    key-switch chunk"""
    E, R = small
    level = 2
    rng = np.random.default_rng(70 + pairs)
    xs = [rand_ct(R.O, level, 2, rng) for _ in range(4)]
    cs = [E.import_ct(x, level) for x in xs]
    idx = [(i % 4, (i * 3 + 1) % 4) for i in range(pairs)]
    want = {ij: R.mul_relin_rescale(level, xs[ij[0]], xs[ij[1]]) for ij in set(idx)}
    got = E.multiply_many([(cs[i], cs[j]) for i, j in idx])
    assert len(got) == pairs
    for m, ij in enumerate(idx):
        assert got[m].level == level - 1
        assert np.array_equal(E.export(got[m]), want[ij]), (m, ij)


def test_galois_multi_mixed_levels_bitexact(small):
    """the batch of test_gpu_low_p.test_mixed_level_batch: a reduced member (level 3) and a two-digit member (level 5),
    rotations and conjugations in one aesfhe_galois_multi call"""
    E, R = small
    rng = np.random.default_rng(8)
    lo, hi = rand_ct(R.O, 3, 2, rng), rand_ct(R.O, 5, 2, rng)
    clo, chi = E.import_ct(lo, 3), E.import_ct(hi, 5)
    rot, conj = E.galois_rotate(2), E.galois_conj
    items = [(clo, 3, lo, rot), (chi, 5, hi, rot), (chi, 5, hi, conj), (clo, 3, lo, conj)]
    got = E.galois_multi([(c, g) for c, _, _, g in items])
    for m, (_, level, x, g) in enumerate(items):
        assert got[m].level == level
        assert np.array_equal(E.export(got[m]), R.galois(level, g, x)), (m, level, g)


@pytest.mark.parametrize("members", [2, 11])
def test_stacked_rotate_bitexact(small, members):
    E, R = small
    level, steps = 1, 5
    rng = np.random.default_rng(90 + members)
    xs = [rand_ct(R.O, level, 2, rng) for _ in range(members)]
    out = E.unstack(E.rotate(E.stack([E.import_ct(x, level) for x in xs]), delta=steps))
    assert len(out) == members
    g = E.galois_rotate(steps)
    for m in range(members):
        assert np.array_equal(E.export(out[m]), R.galois(level, g, xs[m])), m


# ---------------------------------------------------------------------------- the unfused-ModDown fallback
def test_unfused_moddown_fallback_bitexact():
    """max_level 14, dnum 1 (alpha 16): level 13 has no fused ModDown + rescale table, level 12 has"""
    E, R = _pair(14, 1, 0x1A7)
    assert (E.alpha, E.n_p) == (16, 17)
    assert (E.nl(13), E.ks_special_primes(13)) == (15, 16) and (E.nl(12), E.ks_special_primes(12)) == (14, 15)
    rng = np.random.default_rng(10)
    for level in (13, 12):
        assert np.array_equal(E.export_ksk_at(0, level), R.low_key(0, level)), level
        _check_mul(E, R, level, rng)


# ---------------------------------------------------------------------------- N = 2^16, the C2 7/4 set
@pytest.fixture(scope="module")
def c2():
    from engine_context import EngineContext
    from oracle.ckks_cpu import OracleParams
    ctx = EngineContext(signature=1, boot_fresh_level=7, dnum=4, thread_count=4, seed=0xC2C2, enc_nonce=0xC2C2)
    E = ctx.engine
    assert E.low_p and (E.alpha, E.n_p) == (10, 11)
    # the engine's chain (tests/test_gpu_boot_parity.py): single-prime levels up to L1, double-prime levels above
    L1 = max(l for l in range(E.L + 1) if E.level_limbs[l] == l + 2)
    O = OracleParams(log_n=16, max_level=L1, dnum=E.dnum, seed=0xC2C2, boot_double=E.L - L1)
    assert np.array_equal(E.moduli(), O.moduli)
    assert [O.nl(l) for l in range(O.L + 1)] == E.level_limbs
    assert (E.ks_special_primes(1), E.ks_special_primes(7)) == (4, 10)
    return E, Ref(O)


@pytest.mark.parametrize("which", ["relin", "conj"])
def test_c2_keys_and_keyswitch_bitexact(c2, which):
    E, R = c2
    g = _tags(E)[which]
    assert np.array_equal(E.export_ksk_at(g, 7), R.low_key(g, 7))
    rng = np.random.default_rng(11)
    for level in (1, 7):
        d = rand_rows(R.O, E.nl(level), rng)
        assert np.array_equal(E.debug_keyswitch(level, g, d), R.O.keyswitch_low(level, [d], [R.low_key(g, level)])), level


def test_c2_multiply_relin_rescale_bitexact(c2):
    E, R = c2
    _check_mul(E, R, 7, np.random.default_rng(12))
