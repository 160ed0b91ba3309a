"""Typed value decode (aesfhe_xor_value_typed) against the CPU oracle and the integer models.

* encode parity: the G x 16 weighted coefficient plaintexts of the device codec (k_value_slots_typed -> inverse FFT ->
  untwist -> NTT) against the oracle's host encoding of the same slot vectors, at both FFT pass splits;
* bit-exact: every T_g and R_g equals sum_t A_t (.) P_{g,t} mod q put through the oracle's rescale, word for word, and
  with one group, unit weights and no flags they equal xor_value_public's outputs;
* the refusals; all 256 nibble pairs at log N 15 for "i1" and ">i2" with per-slot gains;
* AESPipeline.transcipher_values with dtype / gain / offset on the C2 set of tests/test_gpu_ctr.py.

Value errors are in LSB units of the word's lowest byte: (decoded - gain * q - offset) / |gain|.  8-bit types ask
< 0.25 (the project's bound for the secret-key renorm cases); a 16-bit word's error is its low byte's plus 256 times
its top byte's, so the same per-byte bound through the word weights is 257 * 0.25.  Slots that hold no word are
measured against the smallest |gain| in use.  The measured figures are in DESIGN.md §3.21.
"""
import numpy as np
import pytest

from conftest import gpu_context
from test_gpu_lut import rand_ct
from test_gpu_xor_value import NONCE, _block_fn, _expected, _operands, _tables, co, ctx9, pair, rks, small  # noqa: F401

pytestmark = pytest.mark.gpu

BOUND = {1: 0.25, 2: 257 * 0.25}


def _weights(E, rng, groups):
    """weights in [-1/128, 1/128] with a third of the slots at 0, flags on a quarter of the slots"""
    sc = E.slot_count
    w = rng.uniform(-1.0 / 128.0, 1.0 / 128.0, (groups, sc))
    w[rng.random((groups, sc)) < 1.0 / 3.0] = 0.0
    f = (rng.random((groups, sc)) < 0.25).astype(np.uint8)
    return np.ascontiguousarray(w), np.ascontiguousarray(f)


def _slot_values(tabs, nib, w, f, half, p):
    """the slot vector of channel (half, p): weight * table entry, the hi half's odd rows negated on flagged slots"""
    v = w * tabs[half][p, nib[half]]
    return np.where((f & 1).astype(bool), -v, v) if half == 0 and p % 2 else v


def test_typed_encode_parity(pair):
    """Device rows vs OracleParams.encode of the same weighted table values: |w| <= 1/128 keeps every value below 1
    (16 * 2.563 / 128 = 0.32), so test_value_encode_parity's bound and reason apply: at most 1 per coefficient, the
    same integer on every limb."""
    E, O = pair
    level = min(O.L, 5)
    nl = E.nl(level)
    rng = np.random.default_rng(81)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    w, f = _weights(E, rng, 2)
    tabs = _tables(1.0)
    rows, scale = E.debug_xor_value_typed_pt(nib[0], nib[1], w, f, level)
    assert rows.shape == (2, 16, nl, O.n)
    q = O.limbs_mod(nl).astype(np.int64).reshape(-1, 1)
    worst = 0
    for g in range(2):
        for t in range(16):
            half, p = t // 8, t % 8 + 1
            dev = O.intt(rows[g, t], range(nl)).astype(np.int64)
            ref = O.intt(O.encode(_slot_values(tabs, nib, w[g], f[g], half, p), scale, nl), range(nl)).astype(np.int64)
            d = (dev - ref) % q
            d = np.where(d > q // 2, d - q, d)
            worst = max(worst, int(np.abs(d).max()))
            assert np.abs(d).max() <= 1, (g, t, int(np.abs(d).max()))
            assert np.all(d == d[0])  # one integer per coefficient, the same on every limb
    print(f"log N {O.log_n}: max |device - oracle| coefficient = {worst} at scale 2^{np.log2(scale):.2f}")


@pytest.mark.parametrize("groups", [1, 2])
def test_typed_mac_bitexact(small, groups):
    E, O = small
    rng = np.random.default_rng(82 + groups)
    a_hi, a_lo, l = _operands(E, O, rng, 6)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    w, f = _weights(E, rng, groups)
    out = E.xor_value_typed(a_hi, a_lo, nib[0], nib[1], w, f)
    assert len(out) == groups
    P = E.debug_xor_value_typed_pt(nib[0], nib[1], w, f, l)[0]
    ops = [(a, 8 * half + p - 1, p) for half, A in enumerate((a_hi, a_lo)) for p, a in sorted(A.items())]
    for g, (T, R) in enumerate(out):
        assert T.level == R.level == l - 1
        assert np.array_equal(E.export(T), _expected(E, O, [(a, t) for a, t, p in ops if p <= 7], P[g], l)), g
        assert np.array_equal(E.export(R), _expected(E, O, [(a, t) for a, t, p in ops if p == 8], P[g], l)), g


def test_typed_unit_weights_equal_public(small):
    """one group, unit weights, no flags: the same words as xor_value_public on the unit tables"""
    E, O = small
    rng = np.random.default_rng(85)
    a_hi, a_lo, l = _operands(E, O, rng, 6)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    (T, R), = E.xor_value_typed(a_hi, a_lo, nib[0], nib[1], np.ones(E.slot_count))
    T0, R0 = E.xor_value_public(a_hi, a_lo, nib[0], nib[1], *_tables(1.0))
    assert T.level == T0.level and R.level == R0.level
    assert np.array_equal(E.export(T), E.export(T0))
    assert np.array_equal(E.export(R), E.export(R0))
    assert np.array_equal(E.debug_xor_value_typed_pt(nib[0], nib[1], np.ones(E.slot_count), None, l)[0][0],
                          E.debug_xor_value_pt(nib[0], nib[1], *_tables(1.0), l)[0])


def test_typed_errors(small):
    E, O = small
    rng = np.random.default_rng(86)
    sc = E.slot_count
    nib = rng.integers(0, 16, sc).astype(np.uint8)
    w = np.full((2, sc), 1.0 / 256.0)
    a_hi = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in range(1, 9)}
    a_lo = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in range(1, 9)}
    bad = nib.copy()
    bad[sc // 2] = 16
    with pytest.raises(RuntimeError, match="nibble"):
        E.xor_value_typed(a_hi, a_lo, nib, bad, w)
    with pytest.raises(RuntimeError, match="slot_count"):
        E.xor_value_typed(a_hi, a_lo, nib[:-1].copy(), nib[:-1].copy(), w[:, :-1])
    with pytest.raises(RuntimeError, match="level"):
        E.xor_value_typed({p: E.import_ct(rand_ct(O, 0, rng), 0) for p in range(1, 9)}, a_lo, nib, nib, w)
    with pytest.raises(RuntimeError, match="stack"):
        E.xor_value_typed({**a_hi, 3: E.stack([a_hi[3], a_hi[5]])}, a_lo, nib, nib, w)
    with pytest.raises(RuntimeError, match="used row"):
        E.xor_value_typed(a_hi, {p: a_lo[p] for p in range(1, 8)}, nib, nib, w)
    with pytest.raises(RuntimeError, match="n_groups"):
        E.xor_value_typed(a_hi, a_lo, nib, nib, np.ones((3, sc)))
    for poison in (np.nan, np.inf):
        wb = w.copy()
        wb[1, sc - 1] = poison
        with pytest.raises(RuntimeError, match="weight not finite"):
            E.xor_value_typed(a_hi, a_lo, nib, nib, wb)
    with pytest.raises(RuntimeError, match="missing weights"):
        E.xor_value_typed(a_hi, a_lo, nib, nib, None)
    out = E.xor_value_typed(a_hi, a_lo, nib, nib, w)  # the handles are intact after the refused calls
    assert [c.level for pr in out for c in pr] == [2, 2, 2, 2]


def _want(st, dtype):
    return np.ascontiguousarray(st).view(np.dtype(dtype)).astype(np.float64)


def _check_typed(enc, ct, m, dtype, gain, offset, what, slots=None):
    """decoded words within the bound of gain * q + offset, every other slot within it of 0; prints the figures"""
    from state_encoder import value_dtype
    w = value_dtype(dtype)[0]
    states, nw = m.shape[0], 16 // w
    g, off = np.broadcast_to(gain, (states, nw)), np.broadcast_to(offset, (states, nw))
    z = enc.ctx.decrypt(ct) if slots is None else slots
    got = enc.values_from_slots(z, dtype).reshape(states, nw)
    err = float(np.abs((got - g * _want(m, dtype) - off) / g).max())
    word = np.zeros((states, 16))
    word[:, ::w] = 1.0
    rest = enc._float_slots(word) == 0.0
    stray = float(np.abs(z[rest]).max() / np.abs(g).min()) if rest.any() else 0.0
    print(f"{what}: max value error {err:.3g} LSB, other slots {stray:.3g} LSB (bound {BOUND[w]}), "
          f"max |imag| {np.abs(z.imag).max() / np.abs(g).min():.3g} LSB")
    assert err < BOUND[w] and stray < BOUND[w]
    return got, g, off


@pytest.mark.parametrize("dtype", ["i1", ">i2"])
def test_typed_all_pairs_logn15(dtype):
    """all 256 (state nibble, public nibble) pairs on both halves, test_xor_value_all_pairs_logn15's shapes"""
    import mi355x_ckks
    from state_encoder import StateEncoder, value_dtype
    from utils import XOR_VALUE_DEPTH
    from xor_value_lut import TypedValueLUT
    ctx = gpu_context(log_n=15)
    enc = StateEncoder(ctx, 16)
    w = value_dtype(dtype)[0]
    rng = np.random.default_rng(87)
    gain = rng.choice([-1.0, 1.0], (16, 16 // w)) * rng.uniform(0.5, 2.0, (16, 16 // w)) * 256.0 ** -w
    offset = rng.uniform(-1.0, 1.0, (16, 16 // w))
    state = np.tile(np.arange(16, dtype=np.uint8) * 17, (16, 1))          # state b, byte i: both nibbles i
    public = np.repeat(np.arange(16, dtype=np.uint8) * 17, 16).reshape(16, 16)  # state b: both nibbles b
    lut = TypedValueLUT(ctx, enc.value_slots((dtype, gain, offset)))
    hi, lo = enc.encode(state)
    n0 = mi355x_ckks.launch_count()
    out = lut.apply_public(hi, lo, *enc.nibble_slots(public))
    ctx.engine.settle(out)
    n_val = mi355x_ckks.launch_count() - n0
    assert out.level == hi.level - XOR_VALUE_DEPTH
    got, g, off = _check_typed(enc, out, state ^ public, dtype, gain, offset, f"typed value decode {dtype}, log N 15")
    if w == 1:
        assert np.array_equal(np.rint((got - off) / g), _want(state ^ public, dtype))
    print(f"launch census, typed value decode {dtype} at log N 15: {n_val} launches")


def test_transcipher_values_typed(ctx9, co, rks):
    """4 states across the counter wrap: "<i2" with per-state gains and an offset, "i1" rounding to the integers"""
    import mi355x_ckks
    from ctr_mode import ctr_xor
    from pipeline import AESPipeline
    from utils import XOR_VALUE_DEPTH
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=4)
    rng = np.random.default_rng(88)
    m = rng.integers(0, 256, (4, 16)).astype(np.uint8)
    m[0, :8] = [0x00, 0x80, 0xFF, 0x7F, 0xFF, 0x00, 0x80, 0x7F]
    c0 = 2 ** 32 - 2
    c = ctr_xor(_block_fn(rks), m, NONCE, c0)
    ks_level = pipe.ctr_keystream(NONCE, c0, rks)[0].level
    gain = np.array([[1.0], [-0.5], [2.0], [-1.5]]) / 65536.0
    out = pipe.transcipher_values(c, NONCE, c0, rks, dtype="<i2", gain=gain, offset=0.125)
    assert out.level == ks_level - XOR_VALUE_DEPTH
    assert out.value_dtype == "<i2"
    _check_typed(pipe.encoder, out, m, "<i2", gain, 0.125, "transcipher_values <i2, 4 states across the wrap")
    assert pipe.encoder.decode_values(out).shape == (4, 8)
    with pytest.raises(ValueError):
        pipe.encoder.decode_values(out, ">i2")
    g1 = np.linspace(0.5, 2.0, 16) * np.where(np.arange(16) % 2, -1.0, 1.0) / 256.0
    out = pipe.transcipher_values(c, NONCE, c0, rks, dtype="i1", gain=g1, offset=-0.5)
    assert out.level == ks_level - XOR_VALUE_DEPTH
    got, g, off = _check_typed(pipe.encoder, out, m, "i1", g1, -0.5, "transcipher_values i1, 4 states across the wrap")
    assert np.array_equal(np.rint((got - off) / g), _want(m, "i1"))
    # launch census of the last step alone (printed, not asserted): the typed decode against today's
    ks = pipe.ctr_keystream(NONCE, c0, rks)
    nib = pipe.encoder.nibble_slots(c)
    eng = ctx9.engine
    eng.settle(*ks)
    n = [mi355x_ckks.launch_count()]
    for lut in (pipe._value_lut(1.0 / 256.0), pipe._typed_lut("i1", g1, -0.5), pipe._typed_lut("<i2", gain, 0.125)):
        eng.settle(lut.apply_public(*ks, *nib))
        n.append(mi355x_ckks.launch_count())
    print(f"launch census, last step on the C2 set: u1 scalar gain {n[1] - n[0]}, i1 per-word gain {n[2] - n[1]}, <i2 {n[3] - n[2]} launches")


def test_transcipher_values_typed_fips(ctx9, co, rks):
    """byte_order="transposed": the two bytes of a word sit 4 units apart, so the rotation differs"""
    from ctr_mode import ctr_xor, fips_block_fn
    from pipeline import AESPipeline
    from utils import XOR_VALUE_DEPTH
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True, states=4)
    assert pipe.encoder.word_distance == 4 * pipe.layout.unit
    m = np.random.default_rng(89).integers(0, 256, (4, 16)).astype(np.uint8)
    m[0, :6] = [0x80, 0x00, 0x00, 0xFF, 0xFF, 0x00]
    c0 = 2 ** 32 - 3
    c = ctr_xor(fips_block_fn(rks), m, NONCE, c0)
    ks_level = pipe.ctr_keystream(NONCE, c0, rks)[0].level
    gain = np.linspace(1.0, 2.0, 8) / 65536.0
    out = pipe.transcipher_values(c, NONCE, c0, rks, dtype=">u2", gain=gain, offset=0.25)
    assert out.level == ks_level - XOR_VALUE_DEPTH
    _check_typed(pipe.encoder, out, m, ">u2", gain, 0.25, "transcipher_values >u2, fips, 4 states across the wrap")
