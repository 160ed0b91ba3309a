"""CPU checks of the oracle's reduced-basis key switch (oracle/ckks_oracle.c orc_gen_ksk_low / orc_keyswitch_low,
DESIGN.md §3.3), the reference tests/test_gpu_low_p_parity.py compares the HIP engine with residue for residue: it
has to be right before a kernel is compared with it.

Set: N = 2^13, max_level 10, dnum 2 -> n_ks = 12, alpha = 6, n_p = 7; levels 0..3 (nl = 2..5 < alpha) are reduced,
each over Q_l P_l with P_l = the first nl + 1 special primes.

- key validity: b + a s - (P_l mod q_t) s' on the Q rows and b + a s on the P rows are the NTT of ONE small
  polynomial e: the same centred coefficients on every row, |e_k| <= 21 (the CBD range);
- switch correctness: for uniform d, out0 + out1 s - d s' is small.  The bound is derived: the ModDown's rounding
  contributes at most (1 + ||s||_1) / 2 <= (N + 1) / 2; the conversion term d~ e / P_l is at most
  N * 21 * 1.5 Q_l / P_l < 1 per source since P_l / Q_l > 2^29 (d~ = the centred lift of d, |d~| <= 1.5 Q_l with the
  approximate overflow count); so max |coefficient| <= N.  A wrong table lands near Q_l.
  Measured maxima (printed per (g, level)): 75 .. 92 for one source, 79 .. 83 for two (N = 8192);
- two sources (the conjugation of a deferred 3-polynomial tensor: keys sigma(s) -> s and sigma(s)^2 -> s) are summed
  in Q_l P_l before the one ModDown: the same bound, and the result differs from the sum of two one-source calls by
  at most one per residue -- and does differ somewhere, so the test cannot pass on the wrong composition.
"""
import numpy as np
import pytest

LOG_N, LMAX, DNUM, SEED = 13, 10, 2, 0x10F
REDUCED = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def O():
    from oracle.ckks_cpu import OracleParams
    o = OracleParams(log_n=LOG_N, max_level=LMAX, dnum=DNUM, seed=SEED)
    assert (o.n_ks, o.alpha, o.n_p) == (12, 6, 7)
    return o


@pytest.fixture(scope="module")
def S(O):
    return O.secret_ntt()


def _tags(O):
    return {"relin": 0, "conj": O.galois_conj, "rot1": O.galois_rotate(1), "conj_sq": 4 * O.n + O.galois_conj}


def _mulm(a, b, q):
    return (a.astype(np.uint64) * b.astype(np.uint64)) % q


def _source(O, S, g, nl):
    """s' of tag g on Q limbs 0..nl-1 (NTT form), from the oracle's secret and automorphism only"""
    q = O.limbs_mod(nl)
    s = S[:nl]
    if g == 0:
        return _mulm(s, s, q).astype(np.uint32)
    if g > 4 * O.n:
        return O.automorph(nl - 2, g - 4 * O.n, _mulm(s, s, q).astype(np.uint32)[None])[0]
    return O.automorph(nl - 2, g, s[None])[0]


def _centred(O, rows, limbs):
    """coefficient form of NTT rows on the global primes `limbs`, centred per row: int64 [rows][N]"""
    c = O.intt(rows, limbs).astype(np.int64)
    q = O.moduli[list(limbs)].astype(np.int64)[:, None]
    return np.where(c > q // 2, c - q, c)


def _rand_rows(O, nl, rng):
    return np.stack([rng.integers(0, int(O.moduli[t]), O.n, dtype=np.uint64) for t in range(nl)]).astype(np.uint32)


def _noise(O, S, level, out, terms):
    """max |out0 + out1 s - sum d s'| over the coefficients; the centred value must be one integer on every limb"""
    nl = O.nl(level)
    q = O.limbs_mod(nl)
    r = (out[0].astype(np.uint64) + _mulm(out[1], S[:nl], q)) % q
    for d, sp in terms:
        r = (r + q - _mulm(d, sp, q)) % q
    c = _centred(O, r.astype(np.uint32), range(nl))
    assert np.all(c == c[0]), "the noise is not one small integer polynomial on every limb"
    return int(np.abs(c[0]).max())


def test_refused_off_the_reduced_levels(O):
    with pytest.raises(ValueError):
        O.gen_ksk_low(0, 4)  # nl = alpha: the full key serves
    with pytest.raises(ValueError):
        O.keyswitch_low(4, [np.zeros((6, O.n), np.uint32)], [np.zeros((2, 13, O.n), np.uint32)])


@pytest.mark.parametrize("which", ["relin", "conj", "rot1", "conj_sq"])
def test_reduced_key_is_an_rlwe_sample_of_the_gadget(O, S, which):
    g = _tags(O)[which]
    for level in REDUCED:
        nl, np_l = O.nl(level), O.nl(level) + 1
        key = O.gen_ksk_low(g, level)
        assert key.shape == (2, nl + np_l, O.n)
        limbs = list(range(nl)) + [O.n_q + k for k in range(np_l)]
        q = O.moduli[limbs].astype(np.uint64)[:, None]
        r = (key[0].astype(np.uint64) + _mulm(key[1], S[limbs], q)) % q
        P = 1
        for k in range(np_l):
            P *= int(O.moduli[O.n_q + k])
        pmod = np.array([[P % int(O.moduli[t])] for t in range(nl)], np.uint64)
        r[:nl] = (r[:nl] + q[:nl] - _mulm(pmod, _source(O, S, g, nl), q[:nl])) % q[:nl]
        e = _centred(O, r.astype(np.uint32), limbs)
        assert np.abs(e).max() <= 21, (which, level, int(np.abs(e).max()))
        assert np.all(e == e[0]), (which, level)
        assert np.any(e[0] != 0)
        # fresh randomness per level: the a parts of two levels differ on their shared rows
        if level > REDUCED[0]:
            assert not np.array_equal(key[1][:2], O.gen_ksk_low(g, level - 1)[1][:2])


@pytest.mark.parametrize("which", ["relin", "conj", "rot1", "conj_sq"])
def test_one_source_switch_noise_within_derived_bound(O, S, which):
    g = _tags(O)[which]
    rng = np.random.default_rng(21)
    for level in REDUCED:
        nl = O.nl(level)
        d = _rand_rows(O, nl, rng)
        out = O.keyswitch_low(level, [d], [O.gen_ksk_low(g, level)])
        worst = _noise(O, S, level, out, [(d, _source(O, S, g, nl))])
        print(f"low-P oracle switch {which:8s} level {level}: max |noise coefficient| {worst}")
        assert worst <= O.n, (which, level, worst)
        if g == 0:
            # the same through the oracle's own decryption of the 3-polynomial (out0, out1, -d)
            neg = ((O.limbs_mod(nl) - d) % O.limbs_mod(nl)).astype(np.uint32)
            m = O.decrypt_coeffs(level, np.stack([out[0], out[1], neg]), S)
            assert int(np.abs(m).max()) == worst


def test_two_sources_are_summed_before_the_one_moddown(O, S):
    g = O.galois_conj
    rng = np.random.default_rng(22)
    for level in REDUCED:
        nl = O.nl(level)
        q = O.limbs_mod(nl)
        x = O.automorph(level, g, np.stack([_rand_rows(O, nl, rng) for _ in range(3)]))
        k1, k2 = O.gen_ksk_low(g, level), O.gen_ksk_low(4 * O.n + g, level)
        both = O.keyswitch_low(level, [x[1], x[2]], [k1, k2])
        worst = _noise(O, S, level, both, [(x[1], _source(O, S, g, nl)), (x[2], _source(O, S, 4 * O.n + g, nl))])
        print(f"low-P oracle two-source switch level {level}: max |noise coefficient| {worst}")
        assert worst <= O.n, (level, worst)
        sep = (O.keyswitch_low(level, [x[1]], [k1]).astype(np.uint64) + O.keyswitch_low(level, [x[2]], [k2])) % q
        # coefficient form: the two roundings differ by -1, 0 or 1 in the integers, the same on every limb
        diff = (_centred(O, both.reshape(2 * nl, O.n), list(range(nl)) * 2)
                - _centred(O, sep.astype(np.uint32).reshape(2 * nl, O.n), list(range(nl)) * 2))
        qq = np.concatenate([q, q]).astype(np.int64)
        diff = (diff + qq // 2) % qq - qq // 2
        assert np.abs(diff).max() <= 1, (level, int(np.abs(diff).max()))
        assert np.any(diff != 0), level
        assert not np.array_equal(both, sep.astype(np.uint32))
