"""The edge-residue rows of tests/helpers/edge_patterns.py are what they claim (no GPU): below their moduli,
`conv_top` makes every base-conversion source q_i - 1, `ntt_top` transforms to all q - 1."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import edge_patterns as ep  # noqa: E402


@pytest.fixture(scope="module")
def O():
    from oracle.ckks_cpu import OracleParams
    return OracleParams(log_n=13, max_level=13, dnum=1, seed=0x5EED)  # alpha = 15, 16 special primes


def test_patterns_below_moduli(O):
    q = O.moduli
    pats = ep.basic(q, O.n, 7)
    assert set(pats) == set(ep.BASIC)
    pats["uniform"] = ep.uniform(q, O.n, 7)
    pats["ntt_top_fwd"], pats["ntt_top_inv"] = ep.ntt_top(O, range(len(q)))
    pats["conv_top"] = ep.conv_top_digits(O, O.n_ks, O.alpha)
    for name, x in pats.items():
        assert x.dtype == np.uint32 and x.shape[1] == O.n, name
        assert (x < q[: x.shape[0], None]).all(), name


def test_pattern_contents(O):
    q = O.moduli.astype(np.int64)[:, None]
    p = ep.basic(O.moduli, O.n, 7)
    assert not p["zero"].any()
    assert (p["top"] == q - 1).all()
    assert not p["alt"][:, 0::2].any() and (p["alt"][:, 1::2] == q - 1).all()
    assert (p["alt"].astype(np.int64) + p["alt_c"] == q - 1).all()
    for name, k in zip(ep.IMPULSES, (0, O.n // 2, O.n - 1)):
        assert (p[name][:, k] == q[:, 0] - 1).all() and np.count_nonzero(p[name]) == len(q), name
    # corners: only the seven listed values, and every one of them present in every row
    v = ep.corner_values(O.moduli)
    assert (v[:, 5] + v[:, 6] == q[:, 0]).all()
    for t in range(len(q)):
        assert set(np.unique(p["corners"][t]).tolist()) == set(v[t].tolist()), t
    assert not np.array_equal(p["corners"], ep.corners(O.moduli, O.n, 8))
    assert np.array_equal(p["corners"], ep.corners(O.moduli, O.n, 7))


def test_ntt_top_transforms_to_top(O):
    for limbs in (range(3), range(O.n_q - 2, O.n_q + 2), range(O.n_q + O.n_p)):
        limbs = list(limbs)
        fwd_in, inv_in = ep.ntt_top(O, limbs)
        t = ep.top(O.moduli[limbs], O.n)
        assert np.array_equal(O.ntt(fwd_in, limbs), t)
        assert np.array_equal(O.intt(inv_in, limbs), t)


@pytest.mark.parametrize("limbs", [range(0, 15), range(3, 5), range(7, 8), range(16, 32), range(14, 31)],
                         ids=lambda r: f"{r.start}_{r.stop}")
def test_conv_top_sources_are_q_minus_1(O, limbs):
    limbs = list(limbs)
    q = O.moduli[limbs].astype(np.uint64)[:, None]
    _, inv = ep.conv_weights(O.moduli[limbs])
    coef = O.intt(ep.conv_top(O, limbs), limbs).astype(np.uint64)
    y = coef * np.array(inv, np.uint64)[:, None] % q
    assert (y == q - 1).all()


def test_conv_top_digits_layout(O):
    """digits of alpha limbs, the last one partial: each digit's rows are conv_top of its own limbs"""
    nl, alpha = 11, 4
    d = ep.conv_top_digits(O, nl, alpha)
    assert d.shape == (nl, O.n)
    assert np.array_equal(d[8:11], ep.conv_top(O, range(8, 11)))
    assert np.array_equal(d[4:8], ep.conv_top(O, range(4, 8)))


def test_plaintext_builders(O):
    """pt_top / pt_impulse / pt_small: slot vectors that are non-constant by exact equality and encode, at the scale
    they were built for, to the polynomial they return (tests/test_oracle_hoisted.py runs every row and level)"""
    level = 5
    sc = ep.pt_scale(O.deltas, O.moduli, level)
    assert sc == O.deltas[level - 1] * float(O.moduli[level + 1]) / O.deltas[level]  # csrc/params.cpp ptscale[l]
    nl = O.nl(level)
    limbs = list(range(nl)) + list(range(O.n_q, O.n_q + O.n_p))
    built = {"top": ep.pt_top(O, sc), "impulse": ep.pt_impulse(O, sc), "small": ep.pt_small(O, sc, 3)}
    for name, (z, m) in built.items():
        assert z.dtype == np.complex128 and z.shape == (O.slot_count,) and m.dtype == np.int64 and m.shape == (O.n,), name
        assert not (z == z[0]).all(), name
        assert np.array_equal(O.encode_ext(z, sc, nl, O.n_p), ep.poly_ntt(O, m, limbs)), name
    z, m = built["top"]
    assert m[0] == -1 and not m[1:].any()
    assert np.allclose(z * sc, -1.0, rtol=1e-11, atol=0) and np.count_nonzero(z != z[0]) == 1  # one nudged slot
    assert np.array_equal(ep.poly_ntt(O, m, limbs), ep.top(O.moduli[limbs], O.n))
    z, m = built["impulse"]
    assert np.count_nonzero(m) == 1 and m[O.n // 2 + 1] == -1
    enc = ep.poly_ntt(O, m, limbs)
    assert all(len(np.unique(r)) == O.n for r in enc)  # N distinct residues per row: minus the odd powers of psi
    z, m = built["small"]
    assert np.abs(m).max() <= 1 << 20 and len(np.unique(m)) > O.n // 2
    assert np.array_equal(ep.pt_small(O, sc, 3)[1], m) and not np.array_equal(ep.pt_small(O, sc, 4)[1], m)
    with pytest.raises(ValueError):
        ep.pt_from_poly(O, np.zeros(O.n - 1, np.int64), sc)
