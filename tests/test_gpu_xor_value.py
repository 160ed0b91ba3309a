"""Public XOR fused with the value decode (aesfhe_xor_value_public) against the CPU oracle and the
byte models.

* encode parity: the 16 coefficient plaintexts of the device codec (k_value_slots_typed -> inverse FFT -> untwist -> NTT)
  against the oracle's host encoding of the same slot vectors, at both FFT pass splits (log N 13 and 16);
* bit-exact: T and R equal sum_t A_t (.) P_t mod q put through the oracle's rescale, word for word;
* the five refusals; all 256 (state nibble, public nibble) pairs on both halves at log N 15;
* AESPipeline.transcipher_values / to_values on the C2 set of tests/test_gpu_ctr.py and on the 11 / 4 true-FHE set.

Value errors are in BYTE units (the decoded slot divided by the gain, minus the byte): rounding to the right byte
needs < 0.5, the secret-key renorm cases ask < 0.25 (2x room).  The measured figures are in DESIGN.md §3.20.
"""
import numpy as np
import pytest

from conftest import gpu_context, gpu_engine
from test_gpu_lut import rand_ct

pytestmark = pytest.mark.gpu

SETS = [(13, 6), (16, 17)]
GAIN = 1.0 / 256.0
NONCE = bytes(range(0xA0, 0xAC))


def _tables(gain=GAIN):
    from coeffgen import xor_value_table
    E = xor_value_table()[:9]
    return np.ascontiguousarray(16.0 * gain * E), np.ascontiguousarray(gain * E)


@pytest.fixture(scope="module", params=SETS, ids=lambda s: f"logn{s[0]}_L{s[1]}")
def pair(request):
    from oracle.ckks_cpu import OracleParams
    log_n, L = request.param
    return gpu_engine(log_n=log_n, max_level=L, seed=0x5EED), OracleParams(log_n=log_n, max_level=L, dnum=3, seed=0x5EED)


@pytest.fixture(scope="module")
def small():
    from oracle.ckks_cpu import OracleParams
    return gpu_engine(log_n=13, max_level=6, seed=0x5EED), OracleParams(log_n=13, max_level=6, dnum=3, seed=0x5EED)


def test_value_encode_parity(pair):
    """Device rows vs OracleParams.encode of the same table values at the same nibbles: both round the same real
    coefficient vector, the device fp64 FFT's error on values <= 256 * scale ~ 2^38 is ~2^-11 (here the values are
    below 1), so they can only disagree next to a half-integer: at most 1 per coefficient (the same integer on every
    limb) -- tests/test_gpu_public_lut.py's bound and reason."""
    E, O = pair
    level = min(O.L, 5)
    nl = E.nl(level)
    rng = np.random.default_rng(71)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    tabs = _tables()
    rows, scale = E.debug_xor_value_pt(nib[0], nib[1], *tabs, level)
    assert rows.shape == (16, nl, O.n)
    q = O.limbs_mod(nl).astype(np.int64).reshape(-1, 1)
    worst = 0
    for t in range(16):
        half, p = t // 8, t % 8 + 1
        dev = O.intt(rows[t], range(nl)).astype(np.int64)
        ref = O.intt(O.encode(tabs[half][p, nib[half]], scale, nl), range(nl)).astype(np.int64)  # encode returns NTT form
        d = (dev - ref) % q
        d = np.where(d > q // 2, d - q, d)
        worst = max(worst, int(np.abs(d).max()))
        assert np.abs(d).max() <= 1, (t, int(np.abs(d).max()))
        assert np.all(d == d[0])  # one integer per coefficient, the same on every limb
    print(f"log N {O.log_n}: max |device - oracle| coefficient = {worst} at scale 2^{np.log2(scale):.2f}")


def _operands(E, O, rng, top):
    """hi^p / lo^p stand-ins for p = 1..8 at mixed levels, one owing a rescale (a deferred scalar product)"""
    def ct(level):
        return E.import_ct(rand_ct(O, level, rng), level)
    a_hi = {p: ct(top) for p in range(1, 9)}
    a_lo = {p: ct(top) for p in range(1, 9)}
    a_hi[3], a_lo[8] = ct(top - 1), ct(top - 1)
    a_lo[5] = E.multiply(ct(top), 0.625)
    return a_hi, a_lo, top - 1


def _expected(E, O, ops, P, l):
    """sum of export(a_t) (.) P_t over the (operand, channel) pairs `ops`, rescaled by the oracle"""
    nl = E.nl(l)
    q = O.limbs_mod(nl).astype(np.uint64).reshape(1, -1, 1)
    acc = np.zeros((2, nl, O.n), np.uint64)
    for a, t in ops:
        c = a if a.level == l else E.level_down(a, l)
        acc = (acc + E.export(c).astype(np.uint64) * P[t][None].astype(np.uint64) % q) % q
    return O.rescale(l, acc.astype(np.uint32))


def test_value_mac_bitexact(small):
    E, O = small
    rng = np.random.default_rng(72)
    a_hi, a_lo, l = _operands(E, O, rng, 6)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    tabs = _tables()
    T, R = E.xor_value_public(a_hi, a_lo, nib[0], nib[1], *tabs)
    assert T.level == R.level == l - 1
    P = E.debug_xor_value_pt(nib[0], nib[1], *tabs, l)[0]
    ops = [(a, 8 * half + p - 1, p) for half, A in enumerate((a_hi, a_lo)) for p, a in sorted(A.items())]
    assert np.array_equal(E.export(T), _expected(E, O, [(a, t) for a, t, p in ops if p <= 7], P, l))
    assert np.array_equal(E.export(R), _expected(E, O, [(a, t) for a, t, p in ops if p == 8], P, l))


def test_value_errors(small):
    E, O = small
    rng = np.random.default_rng(73)
    tabs = _tables()
    nib = rng.integers(0, 16, E.slot_count).astype(np.uint8)
    a_hi = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in range(1, 9)}
    a_lo = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in range(1, 9)}
    bad = nib.copy()
    bad[E.slot_count // 2] = 16
    with pytest.raises(RuntimeError, match="nibble"):
        E.xor_value_public(a_hi, a_lo, nib, bad, *tabs)
    with pytest.raises(RuntimeError, match="slot_count"):
        E.xor_value_public(a_hi, a_lo, nib[:-1].copy(), nib[:-1].copy(), *tabs)
    with pytest.raises(RuntimeError, match="level"):
        E.xor_value_public({p: E.import_ct(rand_ct(O, 0, rng), 0) for p in range(1, 9)}, a_lo, nib, nib, *tabs)
    with pytest.raises(RuntimeError, match="stack"):
        E.xor_value_public({**a_hi, 3: E.stack([a_hi[3], a_hi[5]])}, a_lo, nib, nib, *tabs)
    with pytest.raises(RuntimeError, match="used row"):
        E.xor_value_public(a_hi, {p: a_lo[p] for p in range(1, 8)}, nib, nib, *tabs)
    T, R = E.xor_value_public(a_hi, a_lo, nib, nib, *tabs)  # the handles are intact after the refused calls
    assert T.level == R.level == 2


def _check_values(enc, ct, want, bound, what, gain=GAIN):
    """decode_values rounds to `want` exactly; the largest error in byte units is printed and below `bound`"""
    got = enc.decode_values(ct) / gain
    want = np.asarray(want)
    err = float(np.abs(got - want).max())
    print(f"{what}: max value error {err:.3g} byte units (bound {bound}, rounding margin 0.5)")
    assert got.shape == want.shape
    assert np.array_equal(np.rint(got).astype(np.int64), want.astype(np.int64))
    assert err < bound
    return err


def test_xor_value_all_pairs_logn15():
    """all 256 (state nibble, public nibble) pairs on both halves, test_xor4_public_all_pairs_logn15's shapes"""
    import mi355x_ckks
    from state_encoder import StateEncoder
    from utils import XOR_VALUE_DEPTH
    from xor_value_lut import XorValueLUT
    ctx = gpu_context(log_n=15)
    enc = StateEncoder(ctx, 16)
    lut = XorValueLUT(ctx, GAIN)
    state = np.tile(np.arange(16, dtype=np.uint8) * 17, (16, 1))          # state b, byte i: both nibbles i
    public = np.repeat(np.arange(16, dtype=np.uint8) * 17, 16).reshape(16, 16)  # state b: both nibbles b
    hi, lo = enc.encode(state)
    n0 = mi355x_ckks.launch_count()
    out = lut.apply_public(hi, lo, *enc.nibble_slots(public))
    ctx.engine.settle(out)  # deferred calls resolved and every owed rescale applied: the census counts the whole op
    n_val = mi355x_ckks.launch_count() - n0
    assert out.level == hi.level - XOR_VALUE_DEPTH
    _check_values(enc, out, state ^ public, 0.25, "public XOR + value decode, log N 15")
    z = ctx.decrypt(out)
    empty = np.ones(ctx.engine.slot_count, bool)
    empty[:16 * enc.stride].reshape(16, enc.stride)[:, :16] = False
    print(f"slots without a state: max |value| {np.abs(z[empty]).max() / GAIN:.3g} byte units; max |imag| {np.abs(z.imag).max() / GAIN:.3g}")
    assert np.abs(z[empty]).max() / GAIN < 0.25
    n0 = mi355x_ckks.launch_count()
    plain = lut.apply(hi, lo)
    ctx.engine.settle(plain)
    n_plain = mi355x_ckks.launch_count() - n0
    _check_values(enc, plain, state, 0.25, "plain value decode, log N 15")
    print(f"launch census, value decode at log N 15: public operand {n_val} launches, zero nibbles {n_plain} launches")


# ---------------------------------------------------------------- the C2 set (tests/test_gpu_ctr.py's fixture)
@pytest.fixture(scope="module")
def ctx9():
    from engine_context import EngineContext
    return EngineContext(signature=1, boot_fresh_level=7, dnum=4, thread_count=4, seed=0xC2C2, enc_nonce=0xC2C2)


@pytest.fixture(scope="module")
def co(coeff_dir):
    from aes_keyschedule import load_all_coeffs
    return load_all_coeffs(coeff_dir)


@pytest.fixture(scope="module")
def rks():
    from aes_keyschedule import expand_aes128_key
    return expand_aes128_key(np.random.default_rng(0xC7).integers(0, 256, 16).astype(np.uint8))


@pytest.fixture(scope="module")
def pipe1(ctx9, co):
    from pipeline import AESPipeline
    return AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)


def _block_fn(rks):
    from oracle import aes_plain
    return lambda blk: aes_plain.ref_encrypt(blk, rks)


def test_transcipher_values_one_state_and_counter_wrap(pipe1, rks):
    import mi355x_ckks
    from ctr_mode import ctr_xor
    from utils import XOR_VALUE_DEPTH
    rng = np.random.default_rng(74)
    fn = _block_fn(rks)
    ks_level = pipe1.ctr_keystream(NONCE, 0, rks)[0].level
    for counter0 in (2 ** 32 - 1, 0):  # the block after counter 2^32 - 1 is counter 0: the second call is the wrap
        m = rng.integers(0, 256, (1, 16)).astype(np.uint8)
        c = ctr_xor(fn, m, NONCE, counter0)
        out = pipe1.transcipher_values(c[0], NONCE, counter0, rks)
        assert out.level == ks_level - XOR_VALUE_DEPTH == 3  # the keystream is not dropped: 3 levels left on this set
        _check_values(pipe1.encoder, out, m[0], 0.25, f"transcipher_values, one state, counter {counter0}")
    # launch census of the last step alone (printed, not asserted): value decode vs public XOR4 + renorm
    ks = pipe1.ctr_keystream(NONCE, 0, rks)
    nib = pipe1.encoder.nibble_slots(c[0])
    eng = pipe1.ctx.engine
    eng.settle(*ks)
    n0 = mi355x_ckks.launch_count()
    eng.settle(pipe1._value_lut(GAIN).apply_public(*ks, *nib))  # settle: deferred calls resolved, owed rescales applied
    n1 = mi355x_ckks.launch_count()
    eng.settle(*pipe1._renorm_pair(*pipe1.ark.public(*ks, *nib, out_level=pipe1._floor())))
    n2 = mi355x_ckks.launch_count()
    print(f"launch census, last step on the C2 set: transcipher_values {n1 - n0} launches, transcipher {n2 - n1} launches")


def test_transcipher_values_64_states(ctx9, co, rks):
    from ctr_mode import ctr_xor
    from pipeline import AESPipeline
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=64)
    assert pipe.layout.periodic
    m = np.random.default_rng(75).integers(0, 256, (64, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 2 ** 32 - 40)  # the 64 counters cross the wrap
    out = pipe.transcipher_values(c, NONCE, 2 ** 32 - 40, rks)
    _check_values(pipe.encoder, out, m, 0.25, "transcipher_values, 64 states across the wrap")


def test_to_values_of_encrypt(pipe1, rks):
    from oracle import aes_plain
    from utils import XOR_VALUE_DEPTH
    pt = np.random.default_rng(76).integers(0, 256, 16).astype(np.uint8)
    hi, lo = pipe1.encrypt(pt, rks)
    out = pipe1.to_values(hi, lo)
    assert out.level == hi.level - XOR_VALUE_DEPTH
    _check_values(pipe1.encoder, out, aes_plain.ref_encrypt(pt, rks), 0.25, "to_values(encrypt)")


def test_transcipher_values_encrypted_round_keys(pipe1, rks):
    from ctr_mode import ctr_xor
    from key_expansion import EncryptedRoundKeys
    erk = EncryptedRoundKeys.from_pairs([pipe1.encoder.encode(k) for k in rks], pipe1.layout)
    m = np.random.default_rng(77).integers(0, 256, (1, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 5)
    _check_values(pipe1.encoder, pipe1.transcipher_values(c[0], NONCE, 5, erk), m[0], 0.25, "transcipher_values, EncryptedRoundKeys")


def test_transcipher_values_fips(ctx9, co, rks):
    from ctr_mode import ctr_xor, fips_block_fn
    from pipeline import AESPipeline
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True)
    m = np.random.default_rng(78).integers(0, 256, (1, 16)).astype(np.uint8)
    c = ctr_xor(fips_block_fn(rks), m, NONCE, 9)
    out = pipe.transcipher_values(c[0], NONCE, 9, rks)
    _check_values(pipe.encoder, out, m[0], 0.25, "transcipher_values, fips")
    from state_encoder import StateEncoder
    with pytest.raises(ValueError):  # a transposed value ciphertext never meets a plain encoder
        StateEncoder(ctx9, 1, periodic=pipe.layout.periodic).decode_values(out)


def test_values_pairs_refused(ctx9, co, rks):
    from pipeline import AESPipeline
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, pairs=2)
    blk = np.zeros(16, np.uint8)
    with pytest.raises(ValueError):
        pipe.transcipher_values(blk, NONCE, 0, rks)
    with pytest.raises(ValueError):
        pipe.to_values(None, None)


def test_transcipher_values_true_fhe(co, rks, monkeypatch):
    """the 11 / 4 true-FHE set: one block, the keystream's own bootstrap + snap the last renorm and no secret-key
    call between the key's encryption and the output.  Bytes exact after rounding (error < 0.5); the error is printed"""
    from ctr_mode import ctr_xor
    from engine_context import EngineContext
    from pipeline import AESPipeline
    from test_gpu_true_fhe import _no_secret_renorm
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    pipe = AESPipeline(c12, co, use_hard_renorm_between_steps=False, true_fhe=True)
    assert pipe.encoder.renorm_hook is not None
    m = np.random.default_rng(79).integers(0, 256, (1, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 7)
    pipe._prepare_round_keys(rks)  # the key's encryption is the client's part
    _no_secret_renorm(c12, monkeypatch)
    out = pipe.transcipher_values(c[0], NONCE, 7, rks)
    monkeypatch.undo()
    _check_values(pipe.encoder, out, m[0], 0.5, "transcipher_values, true-FHE 11 / 4 set")
