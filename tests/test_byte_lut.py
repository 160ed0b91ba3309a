"""A 256-entry byte table fused into the value decode, on the host: coeffgen.byte_value_table against
f(x ^ b) over all 256 x 256 pairs, the table's support and symmetries, byte_value_sensitivity, and
xor_value_lut.ByteValueLUT's fallback loop (existing calls only) on the numpy slot context of test_value_typed."""
import numpy as np
import pytest

from test_value_typed import SC, RotCtx, _Pipe
from utils import ZetaEncoder

ORDERS = ["plain", "transposed"]
LAYOUTS = [(1, False), (4, True), (4, False)]
X = np.arange(256)


def mulaw_table() -> np.ndarray:
    """G.711 mu-law: the byte -> its linear sample / 32768, in (-1, 1)"""
    u = X ^ 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return np.where(u & 0x80, -(t - 0x84), t - 0x84) / 32768.0


TABLES = {
    "identity": X / 256.0,
    "relu": np.maximum(X - 256 * (X >= 128), 0) / 128.0,  # ReLU of the byte read as int8, / 128
    "mulaw": mulaw_table(),
    "random": np.random.default_rng(0).uniform(-1.0, 1.0, 256),
}
NAMES = list(TABLES)


@pytest.mark.parametrize("name", NAMES)
def test_formula_all_pairs(name):
    """C_00 + T + conj(T) over K reproduces f(x ^ b) for all 256 x 256 (x, b) to 1e-12"""
    from coeffgen import byte_value_eval, byte_value_table
    f = TABLES[name]
    K, c00 = byte_value_table(f)
    assert K.shape == (9, 16, 256) and abs(c00 - f.mean()) < 1e-14
    x, b = (g.reshape(-1) for g in np.meshgrid(X, X, indexing="ij"))
    F = byte_value_eval(K, c00, b, ZetaEncoder.to_zeta(x >> 4, 16), ZetaEncoder.to_zeta(x & 15, 16))
    assert np.abs(F - f[x ^ b]).max() < 1e-12


def test_table_support_and_symmetries():
    """exactly the stated support: p = 1..7 with every q, p = 0 and 8 with q = 1..7, and the three real halves at
    (0, 8), (8, 8), (8, 0); every other entry is 0 for every public byte"""
    from coeffgen import BYTE_LUT_Q, byte_value_table
    assert BYTE_LUT_Q == tuple(range(-7, 9))
    K, _ = byte_value_table(TABLES["random"])
    allowed = np.zeros((9, 16), bool)
    allowed[1:8, :] = True
    for p in (0, 8):
        for q in range(1, 8):
            allowed[p, q + 7] = True
    allowed[0, 8 + 7] = allowed[8, 8 + 7] = allowed[8, 0 + 7] = True
    assert allowed.sum() == 129
    used = np.abs(K).max(axis=2) > 0.0
    assert np.array_equal(used, allowed)  # a random table fills the whole support
    for p, q in ((0, 8), (8, 8), (8, 0)):
        assert np.all(K[p, q + 7].imag == 0.0)  # the self-conjugate coefficients are real
    # the halves are half of the full coefficient: C_08 etc. computed directly
    f = TABLES["random"]
    zeta = np.exp(-2j * np.pi / 16)
    k, l = np.indices((16, 16))
    for b in (0, 0x5A, 0xFF):
        g = f[16 * (k ^ (b >> 4)) + (l ^ (b & 15))]
        for p, q in ((0, 8), (8, 8), (8, 0)):
            C = (g * zeta ** (-(p * k + q * l))).sum() / 256.0
            assert abs(C.imag) < 1e-14 and abs(K[p, q + 7, b] - 0.5 * C.real) < 1e-14
        C17 = (g * zeta ** (-(1 * k + -7 * l))).sum() / 256.0
        assert abs(K[1, 0, b] - C17) < 1e-14  # q index 0 is q = -7


def test_sensitivity_of_the_identity_table():
    """x / 256 is the byte value decode times 1 / 256: DESIGN.md §3.20 measured 930 per unit codeword error in byte
    units for it, the same perturbation here must agree within 10 %"""
    from coeffgen import byte_value_sensitivity
    s = byte_value_sensitivity(TABLES["identity"])
    print("sensitivity per unit eps:", {n: round(byte_value_sensitivity(TABLES[n]), 2) for n in NAMES})
    assert abs(s - 930.0 / 256.0) < 0.1 * 930.0 / 256.0


def _run(name, order, states, periodic, public, seed, batched=True):
    from state_encoder import StateEncoder
    from utils import BYTE_LUT_DEPTH
    from xor_value_lut import ByteValueLUT
    rng = np.random.default_rng(seed)
    f = TABLES[name]
    ctx = RotCtx(SC, batched)
    enc = StateEncoder(ctx, states, periodic=periodic, byte_order=order)
    m = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    m[0, :4] = (0x00, 0x7F, 0x80, 0xFF)
    gain = rng.uniform(-2.0, 2.0, (states, 16))
    pub = rng.integers(0, 256, (states, 16)).astype(np.uint8) if public else np.zeros((states, 16), np.uint8)
    state = m ^ pub
    weights, const = enc.lut_slots(gain, f.mean())
    lut = ByteValueLUT(ctx, f, weights)
    assert lut.DEPTH == BYTE_LUT_DEPTH == 5 and np.abs(lut.const - const).max() < 1e-15
    hi, lo = enc._pack(enc._order(state) >> 4), enc._pack(enc._order(state) & 0x0F)
    if public:
        out = lut.apply_public(hi, lo, *enc.nibble_slots(pub[0] if states == 1 else pub))
    else:
        out = lut.apply(hi, lo)
    got = enc.values_from_slots(out, "lut").reshape(states, 16)
    assert np.abs(got - gain * f[m]).max() < 1e-9
    rest = enc._float_slots(np.ones((states, 16))) == 0.0
    assert not rest.any() or np.abs(out[rest]).max() < 1e-9  # slots without a state: 0
    assert np.abs(out.imag).max() < 1e-9
    if batched:
        assert [n for kind, n in ctx.calls if kind == "mul"] == [2, 4, 8, 15]  # the bases, then ONE batch of 15 ct x ct
        assert [n for kind, n in ctx.calls if kind == "conj"] == [7, 1]        # conj(lo^1..7) batched, then conj(T)


@pytest.mark.parametrize("public", [True, False], ids=["public", "zero"])
@pytest.mark.parametrize("states,periodic", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_byte_value_lut_fallback(name, order, states, periodic, public):
    _run(name, order, states, periodic, public, seed=100 * states + 10 * public + NAMES.index(name))


def test_byte_value_lut_fallback_unbatched():
    _run("mulaw", "transposed", 4, True, True, seed=5, batched=False)


class _LutPipe(_Pipe):
    """AESPipeline.to_lut on a numpy context"""

    def __init__(self, enc, pairs=1):
        from pipeline import AESPipeline
        super().__init__(enc, pairs)
        for name in ("_byte_lut", "to_lut"):
            setattr(self, name, getattr(AESPipeline, name).__get__(self))


def test_value_errors():
    from coeffgen import byte_value_sensitivity, byte_value_table
    from state_encoder import StateEncoder
    from xor_value_lut import ByteValueLUT
    ctx = RotCtx(SC)
    enc = StateEncoder(ctx, 4, periodic=True)
    f = TABLES["relu"]
    bad_tables = [f[:255], np.tile(f, (2, 1)), np.where(X == 3, np.nan, f), np.where(X == 200, np.inf, f)]
    for bad in bad_tables:
        with pytest.raises(ValueError):
            byte_value_table(bad)
        with pytest.raises(ValueError):
            byte_value_sensitivity(bad)
        with pytest.raises(ValueError):
            ByteValueLUT(ctx, bad, np.ones(SC))
    for bad in (np.ones(SC - 1), np.ones((2, SC)), np.where(np.arange(SC) == 7, np.nan, 1.0), 1.0):
        with pytest.raises(ValueError):
            ByteValueLUT(ctx, f, bad)  # the weights are per slot, finite
    for bad in (np.ones(15), np.ones((3, 16)), np.ones((4, 8)), np.inf, np.full((4, 16), np.nan)):
        with pytest.raises(ValueError):
            enc.lut_slots(bad)

    class _Two:  # an encoder of two pairs without a stacking context: the refusal is lut_slots' own
        pairs = 2
    with pytest.raises(ValueError, match="pairs"):
        StateEncoder.lut_slots(_Two(), 1.0)
    lut = ByteValueLUT(ctx, f, enc.lut_slots(1.0)[0])
    st = np.random.default_rng(6).integers(0, 256, (4, 16)).astype(np.uint8)
    hi, lo = enc._pack(st >> 4), enc._pack(st & 0x0F)
    zero = np.zeros(SC, np.uint8)
    with pytest.raises(ValueError):
        lut.apply_public(hi, lo, np.full(SC, 16, np.uint8), zero)
    with pytest.raises(ValueError):
        lut.apply_public(hi, lo, zero[:-1], zero[:-1])
    pipe = _LutPipe(enc)
    out = pipe.to_lut(hi, lo, f, gain=np.arange(1.0, 17.0))
    assert np.abs(enc.values_from_slots(out, "lut") - np.arange(1.0, 17.0) * f[st]).max() < 1e-9
    for bad in (f[:255], np.tile(f, (2, 1)), np.where(X == 3, np.nan, f)):
        with pytest.raises(ValueError):
            pipe.to_lut(hi, lo, bad)
    with pytest.raises(ValueError):
        pipe.to_lut(hi, lo, f, gain=np.ones((3, 16)))
    with pytest.raises(ValueError):
        _LutPipe(enc, pairs=2).to_lut(hi, lo, f)


def test_lut_tag_decodes_as_bytes_and_other_tags_are_untouched():
    from state_encoder import LUT_VALUE_TAG, VALUE_DTYPES, StateEncoder, tag_value_dtype, value_dtype

    class Ct:
        def __init__(self, slots):
            self.slots = slots

    assert LUT_VALUE_TAG not in VALUE_DTYPES
    with pytest.raises(ValueError):
        value_dtype(LUT_VALUE_TAG)  # no integer dtype: the existing refusals stand
    enc = StateEncoder(RotCtx(SC), 1)
    v = np.linspace(-1.0, 1.0, 16)
    ct = tag_value_dtype(LUT_VALUE_TAG, Ct(enc._float_slots(v[None, :])))
    assert np.abs(enc.decode_values(ct) - v).max() < 1e-15 and enc.decode_values(ct).shape == (16,)
    with pytest.raises(ValueError):
        enc.decode_values(ct, "<u2")  # a contradicting dtype is refused, as for every tag
