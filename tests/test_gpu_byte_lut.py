"""A 256-entry byte table fused into the value decode (aesfhe_byte_lut_public) against the CPU oracle and
the float64 model gain * f[m].

* encode parity of all 16 x 9 rows against OracleParams.encode at both scales (the p = 0 fills sit at the product scale);
* all 16 outputs U_q bit-exact against the oracle MAC, the fill included;
* the refusals, and an intact call after them;
* AESPipeline.to_lut at log N 15 on 16 states covering all 256 byte values, four tables, both layouts;
* AESPipeline.transcipher_lut on the C2 set of tests/test_gpu_ctr.py (fips, 4 states across the 2^32 counter wrap) and on
  the 11 / 4 true-FHE set.

Error bound, in slot units against the float64 model (never the code under test):
    B_f = (0.25 / 256) * S_f / S_id + 6e-4 * max|gain|
S = coeffgen.byte_value_sensitivity, S_id its value for x / 256: the project's per-byte bound of 0.25 LSB scaled by how
much more the table amplifies a codeword error, plus DESIGN.md §3.21's per-ciphertext floor of 3e-4 slot units for the
two key-switched summands T and conj(T).  Slots without a state are asked the second term alone.  The measured figures
are in DESIGN.md §3.23.
"""
import numpy as np
import pytest

from conftest import gpu_context
from test_byte_lut import NAMES, TABLES
from test_gpu_lut import rand_ct
from test_gpu_xor_value import NONCE, _block_fn, co, ctx9, rks, small  # noqa: F401

pytestmark = pytest.mark.gpu

FLOOR = 6e-4  # two key-switched summands at 3e-4 slot units each


def _bound(name, gain_top):
    from coeffgen import byte_value_sensitivity
    s_f, s_id = byte_value_sensitivity(TABLES[name]), byte_value_sensitivity(TABLES["identity"])
    return (0.25 / 256.0) * s_f / s_id + FLOOR * gain_top, (0.25 / 256.0) * s_f / s_id


def _weights(E, rng):
    """one weight per slot in [-2, 2], a quarter of them exactly 0"""
    w = rng.uniform(-2.0, 2.0, E.slot_count)
    w[rng.random(E.slot_count) < 0.25] = 0.0
    return w


def _centred(d, q):
    d = d % q
    return np.where(d > q // 2, d - q, d)


def test_byte_lut_encode_parity(small):
    """all 16 x 9 device rows at log N 13, level 2, vs OracleParams.encode of the same weighted table values: rows
    p = 1..8 at the plaintext scale, the fills p = 0 at the product scale.  At most 1 per coefficient, the same integer
    on every limb"""
    from coeffgen import byte_value_table
    E, O = small
    level = 2
    nl = E.nl(level)
    rng = np.random.default_rng(171)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    w = _weights(E, rng)
    K, _ = byte_value_table(TABLES["random"])  # fills the whole support (the mu-law table is odd: its p = 0 column is 0)
    rows, scale, fill_scale = E.debug_byte_lut_pt(nib[0], nib[1], K, w, level)
    assert rows.shape == (16, 9, nl, O.n)
    assert fill_scale > scale * 2.0 ** 28  # the product scale: ciphertext scale x plaintext scale
    b = 16 * nib[0].astype(np.int64) + nib[1]
    q = O.limbs_mod(nl).astype(np.int64).reshape(-1, 1)
    worst, bits = {0: 0, 1: 0}, {0: 0.0, 1: 0.0}
    bad = []
    for g in range(16):
        for p in range(9):
            sc = fill_scale if p == 0 else scale
            dev = O.intt(rows[g, p], range(nl)).astype(np.int64)
            ref = O.intt(O.encode(w * K[p, g, b], sc, nl), range(nl)).astype(np.int64)  # encode returns NTT form
            d = _centred(dev - ref, q)
            assert bool(np.any(dev)) == bool(np.any(K[p, g]))  # a row of the support is not empty, the others are
            worst[p != 0] = max(worst[p != 0], int(np.abs(d).max()))
            bits[p != 0] = max(bits[p != 0], float(np.log2(1.0 + np.abs(O.embed_inverse(w * K[p, g, b]) * sc).max())))
            if np.abs(d).max() > 1 or not np.all(d == d[0]):
                bad.append((g, p, int(np.abs(d).max()), bool(np.all(d == d[0]))))
    print(f"log N {O.log_n}: max |device - oracle| coefficient = {worst[1]} at scale 2^{np.log2(scale):.2f} (p = 1..8), "
          f"{worst[0]} at the product scale 2^{np.log2(fill_scale):.2f} (the fills); largest coefficient 2^{bits[1]:.1f} / 2^{bits[0]:.1f}")
    assert not bad, bad[:8]


def _operands(E, O, rng, top):
    """hi^p stand-ins for p = 1..8 at mixed levels, one owing a rescale (a deferred scalar product)"""
    def ct(level):
        return E.import_ct(rand_ct(O, level, rng), level)
    a_hi = {p: ct(top) for p in range(1, 9)}
    a_hi[3] = ct(top - 1)
    a_hi[5] = E.multiply(ct(top), 0.625)
    return a_hi, top - 1


def test_byte_lut_mac_bitexact(small):
    """every U_q equals sum_p export(a_p) (.) P[q, p] + P[q, 0] on c0, mod q, put through the oracle's rescale, word for
    word: operands at level 6 and 5, one owing a rescale; weights with zeros"""
    from coeffgen import byte_value_table
    E, O = small
    rng = np.random.default_rng(172)
    a_hi, l = _operands(E, O, rng, 6)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    w = _weights(E, rng)
    assert (w == 0.0).any()
    K, _ = byte_value_table(TABLES["random"])
    U = E.byte_lut_public(a_hi, nib[0], nib[1], K, w)
    assert len(U) == 16
    P = E.debug_byte_lut_pt(nib[0], nib[1], K, w, l)[0]
    nl = E.nl(l)
    q = O.limbs_mod(nl).astype(np.uint64).reshape(1, -1, 1)
    ops = [E.export(a if a.level == l else E.level_down(a, l)).astype(np.uint64) for _, a in sorted(a_hi.items())]
    for g, u in enumerate(U):
        assert u.level == l - 1
        acc = np.zeros((2, nl, O.n), np.uint64)
        for p, a in enumerate(ops, start=1):
            acc = (acc + a * P[g, p][None].astype(np.uint64) % q) % q
        acc[0] = (acc[0] + P[g, 0].astype(np.uint64)) % q[0]  # the fill joins c0
        assert np.array_equal(E.export(u), O.rescale(l, acc.astype(np.uint32))), g


def test_byte_lut_errors(small):
    from coeffgen import byte_value_table
    E, O = small
    rng = np.random.default_rng(173)
    sc = E.slot_count
    K, _ = byte_value_table(TABLES["relu"])
    nib = rng.integers(0, 16, sc).astype(np.uint8)
    w = np.full(sc, 0.5)
    a_hi = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in range(1, 9)}
    bad = nib.copy()
    bad[sc // 2] = 16
    with pytest.raises(RuntimeError, match="nibble"):
        E.byte_lut_public(a_hi, nib, bad, K, w)
    with pytest.raises(RuntimeError, match="nibble"):
        E.byte_lut_public(a_hi, bad, nib, K, w)
    with pytest.raises(RuntimeError, match="slot_count"):
        E.byte_lut_public(a_hi, nib[:-1].copy(), nib[:-1].copy(), K, w[:-1].copy())
    with pytest.raises(RuntimeError, match="level"):
        E.byte_lut_public({p: E.import_ct(rand_ct(O, 0, rng), 0) for p in range(1, 9)}, nib, nib, K, w)
    with pytest.raises(RuntimeError, match="stack"):
        E.byte_lut_public({**a_hi, 3: E.stack([a_hi[3], a_hi[5]])}, nib, nib, K, w)
    with pytest.raises(RuntimeError, match="used row"):
        E.byte_lut_public({p: a_hi[p] for p in range(1, 8)}, nib, nib, K, w)
    for poison in (np.nan, np.inf):
        wb = w.copy()
        wb[sc - 1] = poison
        with pytest.raises(RuntimeError, match="weight not finite"):
            E.byte_lut_public(a_hi, nib, nib, K, wb)
    with pytest.raises(RuntimeError, match="missing weights"):
        E.byte_lut_public(a_hi, nib, nib, K, None)
    Kbad = K.copy()
    Kbad[4, 9, 77] = np.nan
    with pytest.raises(RuntimeError, match="not finite"):
        E.byte_lut_public(a_hi, nib, nib, Kbad, w)
    with pytest.raises(ValueError):
        E.byte_lut_public(a_hi, nib, nib, K[:8], w)
    U = E.byte_lut_public(a_hi, nib, nib, K, w)  # the handles are intact after the refused calls
    assert [u.level for u in U] == [2] * 16


def _check(enc, ct, name, m, gain, what):
    """|decoded - gain f[m]| <= B_f on state slots, <= the floor term elsewhere; the largest errors are printed first.
    ReLU / 128: its step 1 / 128 exceeds 2 B_f, so rounding to the nearest table entry must be exact too"""
    f = TABLES[name]
    gain = np.broadcast_to(np.asarray(gain, np.float64), m.shape)
    top = float(np.abs(gain).max())
    bound, first = _bound(name, top)
    z = enc.ctx.decrypt(ct)
    got = enc.values_from_slots(z, "lut").reshape(m.shape)
    err = float(np.abs(got - gain * f[m]).max())
    rest = enc._float_slots(np.ones(m.shape)) == 0.0
    stray = float(np.abs(z[rest]).max()) if rest.any() else 0.0
    print(f"{what}, {name}: max error {err:.3g} slot units (bound {bound:.3g} = {first:.3g} + {FLOOR * top:.3g}), slots without a state "
          f"{stray:.3g} (bound {FLOOR * top:.3g}), max |imag| {np.abs(z.imag).max():.3g}")
    assert enc.decode_values(ct).shape == ((16,) if enc.states == 1 else m.shape)
    assert err <= bound
    assert stray <= FLOOR * top
    if name == "relu":
        assert np.array_equal(np.rint(got / gain * 128.0), np.rint(f[m] * 128.0))
    return err, stray


@pytest.fixture(scope="module")
def pipes15(co):
    """{periodic: pipeline} at log N 15, 16 states: the periodic layout and the reference one"""
    from pipeline import AESPipeline
    return {per: AESPipeline(gpu_context(log_n=15), co, use_hard_renorm_between_steps=True, states=16, periodic=per) for per in (True, False)}


@pytest.fixture(scope="module")
def pairs15(pipes15):
    """one encrypted pair per layout: 16 states holding a permutation of all 256 byte values"""
    m = np.random.default_rng(174).permutation(256).astype(np.uint8).reshape(16, 16)
    out = {}
    for per, pipe in pipes15.items():
        hi, lo = pipe.encoder.encode(m)
        pipe.ctx.engine.settle(hi, lo)
        out[per] = (hi, lo)
    return m, out


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "reference"])
@pytest.mark.parametrize("name", NAMES)
def test_to_lut_logn15(pipes15, pairs15, name, periodic):
    import mi355x_ckks
    from utils import BYTE_LUT_DEPTH
    pipe = pipes15[periodic]
    m, pairs = pairs15
    hi, lo = pairs[periodic]
    gain = np.random.default_rng(175).uniform(0.5, 1.0, (16, 16)) * np.where(np.arange(16) % 2, -1.0, 1.0)
    n0 = mi355x_ckks.launch_count()
    out = pipe.to_lut(hi, lo, TABLES[name], gain)
    pipe.ctx.engine.settle(out)
    launches = mi355x_ckks.launch_count() - n0
    assert out.level == hi.level - BYTE_LUT_DEPTH and out.value_dtype == "lut"
    _check(pipe.encoder, out, name, m, gain, f"to_lut log N 15, 16 states, {'periodic' if periodic else 'reference'} layout")
    print(f"launch census, to_lut at log N 15: {launches} launches")


@pytest.mark.parametrize("name", ["relu", "mulaw"])
def test_transcipher_lut_fips_wrap(ctx9, co, rks, name):
    """C2 set, fips=True (transposed bytes), 4 states across the 2^32 counter wrap; output level = keystream level - 5"""
    import mi355x_ckks
    from ctr_mode import ctr_xor, fips_block_fn
    from pipeline import AESPipeline
    from utils import BYTE_LUT_DEPTH
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True, states=4)
    rng = np.random.default_rng(176)
    m = rng.integers(0, 256, (4, 16)).astype(np.uint8)
    m[0, :8] = [0x00, 0x80, 0xFF, 0x7F, 0x01, 0x81, 0xFE, 0x7E]
    c0 = 2 ** 32 - 2
    c = ctr_xor(fips_block_fn(rks), m, NONCE, c0)
    gain = rng.uniform(0.5, 1.0, 16)
    ks_level = pipe.ctr_keystream(NONCE, c0, rks)[0].level
    out = pipe.transcipher_lut(c, NONCE, c0, rks, TABLES[name], gain)
    assert out.level == ks_level - BYTE_LUT_DEPTH == 2
    _check(pipe.encoder, out, name, m, gain, "transcipher_lut, C2 set, fips, 4 states across the wrap")
    if name == "mulaw":  # launch census of the last step alone (printed, not asserted)
        ks = pipe.ctr_keystream(NONCE, c0, rks)
        nib = pipe.encoder.nibble_slots(c)
        eng = ctx9.engine
        eng.settle(*ks)
        n0 = mi355x_ckks.launch_count()
        eng.settle(pipe._byte_lut(TABLES[name], gain).apply_public(*ks, *nib))
        n1 = mi355x_ckks.launch_count()
        eng.settle(pipe._value_lut(1.0 / 256.0).apply_public(*ks, *nib))
        n2 = mi355x_ckks.launch_count()
        print(f"launch census, last step on the C2 set: transcipher_lut {n1 - n0} launches, transcipher_values {n2 - n1} launches")


def test_transcipher_lut_true_fhe(co, rks, monkeypatch):
    """the 11 / 4 true-FHE set: one block, the keystream's own bootstrap + snap the last renorm and no secret-key call
    between the key's encryption and the output (test_gpu_xor_value's true-FHE case, through the mu-law table)"""
    from ctr_mode import ctr_xor
    from engine_context import EngineContext
    from pipeline import AESPipeline
    from test_gpu_true_fhe import _no_secret_renorm
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    pipe = AESPipeline(c12, co, use_hard_renorm_between_steps=False, true_fhe=True)
    assert pipe.encoder.renorm_hook is not None
    m = np.random.default_rng(179).integers(0, 256, (1, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 7)
    pipe._prepare_round_keys(rks)  # the key's encryption is the client's part
    _no_secret_renorm(c12, monkeypatch)
    out = pipe.transcipher_lut(c[0], NONCE, 7, rks, TABLES["mulaw"])
    monkeypatch.undo()
    _check(pipe.encoder, out, "mulaw", m, 1.0, "transcipher_lut, true-FHE 11 / 4 set")
