"""Public-operand LUT evaluation (aesfhe_lut_eval_public) against the CPU oracle.

* encode parity: the coefficient plaintexts the device codec makes (k_public_slots -> inverse FFT -> untwist ->
  NTT) against the oracle's host encoding of the same slot vectors, at both FFT pass splits (log N 13 and 16);
* bit-exact: both outputs equal sum_t A_t (.) P_t mod q put through the oracle's rescale, word for word;
* error paths; XOR4 with a public operand over all 256 nibble pairs; the launch census (printed, not asserted).
"""
import numpy as np
import pytest

from conftest import gpu_context, gpu_engine
from test_gpu_lut import rand_ct

pytestmark = pytest.mark.gpu

SETS = [(13, 6), (16, 17)]
ROWS = (1, 3, 5, 7)


@pytest.fixture(scope="module")
def tables(coeff_dir):
    from add_round_key import load_xor4_coeffs
    from xor4_lut import public_tables
    return public_tables(load_xor4_coeffs(coeff_dir / "xor4_coeffs.json"))


@pytest.fixture(scope="module", params=SETS, ids=lambda s: f"logn{s[0]}_L{s[1]}")
def pair(request):
    from oracle.ckks_cpu import OracleParams
    log_n, L = request.param
    return gpu_engine(log_n=log_n, max_level=L, seed=0x5EED), OracleParams(log_n=log_n, max_level=L, dnum=3, seed=0x5EED)


@pytest.fixture(scope="module")
def small():
    from oracle.ckks_cpu import OracleParams
    return gpu_engine(log_n=13, max_level=6, seed=0x5EED), OracleParams(log_n=13, max_level=6, dnum=3, seed=0x5EED)


def test_public_encode_parity(pair, tables):
    """Device rows vs OracleParams.encode of D_t[nib]: both round the same real coefficient vector, the device
    fp64 FFT's error on values <= 256 * scale ~ 2^38 is ~2^-11, so they can only disagree next to a
    half-integer: at most 1 per coefficient (the same integer on every limb)."""
    E, O = pair
    level = min(O.L, 5)
    nl = E.nl(level)
    nib = np.random.default_rng(31).integers(0, 16, E.slot_count).astype(np.uint8)
    lut = E.lut_create(tables.c1)
    rows, scale = E.debug_public_pt(lut, nib, level)
    assert rows.shape == (len(ROWS), nl, O.n)
    q = O.limbs_mod(nl).astype(np.int64).reshape(-1, 1)
    worst = 0
    for t, p in enumerate(ROWS):
        dev = O.intt(rows[t], range(nl)).astype(np.int64)
        ref = O.intt(O.encode(tables.d1[p, nib], scale, nl), range(nl)).astype(np.int64)  # encode returns NTT form
        d = (dev - ref) % q
        d = np.where(d > q // 2, d - q, d)
        worst = max(worst, int(np.abs(d).max()))
        assert np.abs(d).max() <= 1, (p, int(np.abs(d).max()))
        assert np.all(d == d[0])  # one integer per coefficient, the same on every limb
    print(f"log N {O.log_n}: max |device - oracle| coefficient = {worst} at scale 2^{np.log2(scale):.2f}")


def _operands(E, O, rng, top):
    """a[p] for the used rows at mixed levels, one owing a rescale (a deferred scalar product)"""
    a = {1: E.import_ct(rand_ct(O, top, rng), top), 3: E.import_ct(rand_ct(O, top - 1, rng), top - 1),
         5: E.multiply(E.import_ct(rand_ct(O, top, rng), top), 0.625), 7: E.import_ct(rand_ct(O, top, rng), top)}
    return a, top - 1


def _expected(E, O, a, P, l):
    nl = E.nl(l)
    q = O.limbs_mod(nl).astype(np.uint64).reshape(1, -1, 1)
    acc = np.zeros((2, nl, O.n), np.uint64)
    for t, p in enumerate(ROWS):
        c = a[p] if a[p].level == l else E.level_down(a[p], l)
        acc = (acc + E.export(c).astype(np.uint64) * P[t][None].astype(np.uint64) % q) % q
    return O.rescale(l, acc.astype(np.uint32))


@pytest.mark.parametrize("two", [True, False], ids=["lut2", "lut2_none"])
def test_public_mac_bitexact(small, tables, two):
    E, O = small
    rng = np.random.default_rng(32)
    a, l = _operands(E, O, rng, 6)
    nib = rng.integers(0, 16, E.slot_count).astype(np.uint8)
    l1, l2 = E.lut_create(tables.c1), (E.lut_create(tables.c2) if two else None)
    o1, o2 = E.lut_eval_public(l1, l2, a, nib)
    assert o1.level == l - 1 and (o2 is None) == (not two)
    assert np.array_equal(E.export(o1), _expected(E, O, a, E.debug_public_pt(l1, nib, l)[0], l))
    if two:
        assert o2.level == l - 1
        assert np.array_equal(E.export(o2), _expected(E, O, a, E.debug_public_pt(l2, nib, l)[0], l))


def test_public_lut_errors(small, tables):
    E, O = small
    rng = np.random.default_rng(33)
    lut = E.lut_create(tables.c1)
    nib = rng.integers(0, 16, E.slot_count).astype(np.uint8)
    a = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in ROWS}
    bad = nib.copy()
    bad[E.slot_count // 2] = 16
    with pytest.raises(RuntimeError, match="nibble"):
        E.lut_eval_public(lut, None, a, bad)
    with pytest.raises(RuntimeError, match="level"):
        E.lut_eval_public(lut, None, {p: E.import_ct(rand_ct(O, 0, rng), 0) for p in ROWS}, nib)
    with pytest.raises(RuntimeError, match="stack"):
        E.lut_eval_public(lut, None, {**a, 3: E.stack([a[3], a[5]])}, nib)
    with pytest.raises(RuntimeError, match="slot_count"):
        E.lut_eval_public(lut, None, a, nib[:-1].copy())
    with pytest.raises(RuntimeError, match="used row"):
        E.lut_eval_public(lut, None, {1: a[1]}, nib)
    o1, _ = E.lut_eval_public(lut, None, a, nib)  # the handles are intact after the refused calls
    assert o1.level == 2


def test_xor4_public_all_pairs_logn15(coeff_dir):
    """AddRoundKey.public over all 256 (state nibble, public nibble) pairs on both halves: exact bytes, and
    test_config1_add_round_key_logn15's own bounds for the encrypted-operand XOR4 (angle error < MARGIN / 4,
    magnitude 256 to 1e-2); four levels instead of five.  The launch census of both forms is printed."""
    import mi355x_ckks
    from add_round_key import AddRoundKey, load_xor4_coeffs
    from state_encoder import StateEncoder
    from test_gpu_aes import MARGIN
    from utils import PUBLIC_XOR_DEPTH, ZetaEncoder
    from xor4_lut import XOR4LUT
    ctx = gpu_context(log_n=15)
    enc = StateEncoder(ctx, 16)
    ark = AddRoundKey(XOR4LUT(ctx, load_xor4_coeffs(coeff_dir / "xor4_coeffs.json")))
    state = np.tile(np.arange(16, dtype=np.uint8) * 17, (16, 1))          # state b, byte i: both nibbles i
    public = np.repeat(np.arange(16, dtype=np.uint8) * 17, 16).reshape(16, 16)  # state b: both nibbles b
    hi, lo = enc.encode(state)
    n0 = mi355x_ckks.launch_count()
    oh, ol = ark.public(hi, lo, *enc.nibble_slots(public))
    n_pub = mi355x_ckks.launch_count() - n0
    assert oh.level == ol.level == hi.level - PUBLIC_XOR_DEPTH
    assert np.array_equal(enc.decode(oh, ol), state ^ public)
    for ct, want in ((oh, (state ^ public) >> 4), (ol, (state ^ public) & 15)):
        z = enc._take(ctx.decrypt(ct))
        err = float(np.abs(np.angle(z / ZetaEncoder.to_zeta(want, 16))).max())
        print(f"public XOR4: max angle error {err:.3g} rad (bound {MARGIN / 4:.3g}), |z| in [{np.abs(z).min():.3f}, {np.abs(z).max():.3f}]")
        assert err < MARGIN / 4
        assert np.allclose(np.abs(z), 256.0, rtol=1e-2)
    n0 = mi355x_ckks.launch_count()
    eh, el = ark(hi, lo, *enc.encode(public))
    n_enc = mi355x_ckks.launch_count() - n0
    assert np.array_equal(enc.decode(eh, el), state ^ public)
    print(f"launch census, AddRoundKey at log N 15: public operand {n_pub} launches, encode + encrypted operand {n_enc} launches")
