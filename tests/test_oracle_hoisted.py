"""The CPU oracle's key switch taken apart (no GPU): ModUp, inner product and ModDown exported on their own
(oracle/ckks_oracle.c orc_modup / orc_key_inner / orc_moddown) compose to `keyswitch` and to `keyswitch_low` bit for
bit, the inner product's X -> X^g read is the automorphism of every extended row, and the plaintext patterns of
tests/helpers/edge_patterns.py encode to the integer polynomial they name -- the preconditions of
tests/test_gpu_hoisted_parity.py, asserted here so that a GPU failure there is never an encoder or a model
disagreement."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import edge_patterns as ep  # noqa: E402
import keyswitch_shapes_probe as ks  # noqa: E402

D_KINDS = ("top", "corners", "conv_top")


@pytest.fixture(scope="module", params=["A", "B", "C", "D"])
def O(request):
    return ks.oracle(request.param)


def ext_limbs(O, level, np_):
    return list(range(O.nl(level))) + list(range(O.n_q, O.n_q + np_))


def automorph_rows(O, rows, limbs, g):
    """X -> X^g of NTT-form rows on any of the oracle's primes, in the coefficient domain (numpy)"""
    c = O.intt(rows, limbs).astype(np.int64)
    q = O.moduli[list(limbs)].astype(np.int64)[:, None]
    e = np.arange(O.n, dtype=np.int64) * int(g) % (2 * O.n)
    out = np.zeros_like(c)
    out[:, e % O.n] = np.where(e[None, :] < O.n, c, (q - c) % q)
    return O.ntt(out.astype(np.uint32), limbs)


def test_three_steps_equal_keyswitch(O):
    """ModDown(inner(ModUp(d)), g = 1) == keyswitch on the full basis, at the three levels of the shapes test"""
    for kind in ("corners", "top"):
        key = ks.make_key(O, kind, seed=7)
        for level in ks.levels(O):
            nd = O.ks_digits(level)
            assert nd == -(-O.nl(level) // O.alpha)
            for dk in D_KINDS:
                d = ks.make_d(O, level, dk)
                ext = O.modup(level, d)
                assert ext.shape == (nd, O.nl(level) + O.n_p, O.n)
                for j in range(nd):  # the own digit's rows are d's
                    lo, hi = j * O.alpha, min((j + 1) * O.alpha, O.nl(level))
                    assert np.array_equal(ext[j, lo:hi], d[lo:hi]), (level, dk, j)
                got = O.moddown(level, O.key_inner(level, ext, d, key))
                assert np.array_equal(got, O.keyswitch(level, d, key)), (kind, level, dk)


@pytest.mark.parametrize("name", ["A", "B"])
def test_three_steps_equal_keyswitch_low(name):
    """the same wrappers at nl + 1 special primes: one digit, the reduced per-level key's layout.  Sets A and B: sets C
    and D (alpha 2 and 1) have no level below alpha limbs"""
    O = ks.oracle(name)
    lows = [lv for lv in range(O.L + 1) if O.nl(lv) < O.alpha]
    assert lows
    for level in sorted({lows[-1], lows[len(lows) // 2], lows[0]}):
        nl = O.nl(level)
        np_ = nl + 1
        qk = O.ext_moduli(level, np_)
        key = np.stack([ep.corners(qk, O.n, 50 + level), ep.uniform(qk, O.n, 60 + level)])
        assert O.ks_digits(level, np_) == 1
        for dk in D_KINDS:
            d = ep.conv_top(O, range(nl)) if dk == "conv_top" else ks.make_d(O, level, dk)
            ext = O.modup(level, d, np_)
            got = O.moddown(level, O.key_inner(level, ext, d, key, 1, np_), np_=np_)
            assert np.array_equal(got, O.keyswitch_low(level, [d], [key])), (level, dk)


def test_moddown_addends(O):
    level = O.L // 2
    nl = O.nl(level)
    q = O.limbs_mod(nl)
    acc = np.stack([ep.corners(O.ext_moduli(level), O.n, 70), ep.uniform(O.ext_moduli(level), O.n, 71)])
    a0, a1 = ep.top(O.moduli[:nl], O.n), ep.corners(O.moduli[:nl], O.n, 72)
    base = O.moddown(level, acc)
    want = np.stack([(base[0].astype(np.uint64) + a0) % q, (base[1].astype(np.uint64) + a1) % q]).astype(np.uint32)
    assert np.array_equal(O.moddown(level, acc, a0, a1), want)
    assert np.array_equal(O.moddown(level, acc, None, a1)[0], base[0])


def test_galois_read_is_automorphism_of_every_row(O):
    """key_inner(g) == key_inner(g = 1) of the rows and of d each taken through X -> X^g, special-prime rows included;
    the own digit comes from d: an ext whose own rows are scrambled gives the same accumulator"""
    level = O.L // 2
    nl = O.nl(level)
    limbs = ext_limbs(O, level, O.n_p)
    key = ks.make_key(O, "corners", seed=9)
    d = ks.make_d(O, level, "corners")
    ext = O.modup(level, d)
    for g in (O.galois_rotate(3), O.galois_conj, O.galois_rotate(-1)):
        got = O.key_inner(level, ext, d, key, g)
        ext_g = np.stack([automorph_rows(O, e, limbs, g) for e in ext])
        d_g = automorph_rows(O, d, range(nl), g)
        assert np.array_equal(d_g, O.automorph(level, g, d[None])[0])
        assert np.array_equal(got, O.key_inner(level, ext_g, d_g, key))
        assert not np.array_equal(got, O.key_inner(level, ext, d, key))
        scr = ext.copy()
        for j in range(ext.shape[0]):
            scr[j, j * O.alpha: min((j + 1) * O.alpha, nl)] = 0
        assert np.array_equal(got, O.key_inner(level, scr, d, key, g))
    with pytest.raises(ValueError):
        O.key_inner(level, ext, d, key, 4)


def test_plaintext_patterns_encode_exactly(O):
    """encode(embed(m) / scale) has inverse NTT exactly m on every row, Q and P, for m = -1, -X^k and random
    coefficients in +-2^20 -- at the mask scale ptscale[l] and at the fill's product scale delta[l-1] q_{l+1}"""
    for level in sorted({O.L, O.L // 2, 1}):
        nl = O.nl(level)
        limbs = ext_limbs(O, level, O.n_p)
        q = O.moduli[limbs].astype(np.int64)[:, None]
        mask_scale = ep.pt_scale(O.deltas, O.moduli, level)
        assert mask_scale == O.deltas[level - 1] * float(O.moduli[level + 1]) / O.deltas[level]
        fill_scale = float(O.deltas[level - 1]) * float(O.moduli[level + 1])
        for scale in (mask_scale, fill_scale):
            pats = {"top": ep.pt_top(O, scale), "impulse": ep.pt_impulse(O, scale), "impulse_last": ep.pt_impulse(O, scale, O.n - 1),
                    "small": ep.pt_small(O, scale, 80 + level)}
            for name, (z, m) in pats.items():
                assert z.shape == (O.slot_count,) and not np.all(z == z[0]), name
                enc = O.encode_ext(z, scale, nl, O.n_p)
                coef = O.intt(enc, limbs).astype(np.int64)
                coef = np.where(coef > q // 2, coef - q, coef)
                assert np.array_equal(coef, np.broadcast_to(m, coef.shape)), (level, name, scale)
                assert np.array_equal(enc, ep.poly_ntt(O, m, limbs)), (level, name)
                assert np.array_equal(enc[:nl], O.encode(z, scale, nl)), (level, name)
                if name == "top":
                    assert np.array_equal(enc, ep.top(O.moduli[limbs], O.n)), level
