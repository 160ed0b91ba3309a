"""Typed value decode on the host: coeffgen.xor_value_table(signed=True), StateEncoder.value_slots /
values_from_slots / decode_values, and xor_value_lut.TypedValueLUT's fallback (existing calls only) on the numpy slot
context of test_public_xor -- every dtype, both byte orders, per-state and per-word gains of both signs, offsets."""
import numpy as np
import pytest

from test_public_xor import A_ALL, B_ALL, SlotCtx
from utils import ZetaEncoder

DTYPES = ["u1", "i1", "<u2", ">u2", "<i2", ">i2"]
SC = 512
# bytes that pin sign and byte order: 0x80, 0x7F, 0xFF alone and the words 0x8000, 0x7FFF, 0x00FF, 0xFF00 both ways round
PINNED = np.array([0x80, 0x00, 0x7F, 0xFF, 0x00, 0xFF, 0xFF, 0x00, 0x00, 0x80, 0xFF, 0x7F, 0x80, 0x7F, 0xFF, 0xFF], np.uint8)


class RotCtx(SlotCtx):
    """SlotCtx with the rotation of engine_context.EngineContext.rotate (np.roll semantics)"""

    def rotate(self, a, steps):
        self.calls.append(("rot", 1))
        return np.roll(a, steps)

    def decrypt(self, ct):
        return np.asarray(getattr(ct, "slots", ct))


def _want(st, dtype):
    """the integers the bytes of (states, 16) spell in dtype, (states, 16 // w)"""
    return np.ascontiguousarray(st).view(np.dtype(dtype)).astype(np.float64)


def _sval(x):
    return x - 16 * (x >= 8)


def test_signed_value_table():
    from coeffgen import xor_value_table
    E, Es = xor_value_table(), xor_value_table(signed=True)
    a = ZetaEncoder.to_zeta(A_ALL, 16)
    full = sum(Es[p, B_ALL] * a ** p for p in range(16))
    assert np.abs(full - _sval(A_ALL ^ B_ALL)).max() < 1e-12      # all 256 (k, b) pairs
    assert np.all(Es[8].imag == 0.0)                               # row 8 is real
    for p in range(1, 16):
        assert np.abs(Es[16 - p] - np.conj(Es[p])).max() < 1e-12  # the conjugate symmetry is kept
    assert np.abs(Es[0] + 0.5).max() < 1e-12
    assert np.array_equal(Es[1::2], -E[1::2]) and np.array_equal(Es[2::2], E[2::2])  # only the odd rows change
    assert np.array_equal(xor_value_table(signed=False), E)
    T = sum(Es[p, B_ALL] * a ** p for p in range(1, 8))
    assert np.abs(-0.5 + Es[8, B_ALL] * a ** 8 + T + np.conj(T) - _sval(A_ALL ^ B_ALL)).max() < 1e-12


def _run(dtype, states, order, periodic, gain_kind, seed, batched=True):
    from state_encoder import StateEncoder, value_dtype
    from xor_value_lut import TypedValueLUT
    rng = np.random.default_rng(seed)
    ctx = RotCtx(SC, batched)
    enc = StateEncoder(ctx, states, periodic=periodic, byte_order=order)
    w = value_dtype(dtype)[0]
    nw = 16 // w
    m = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    m[0] = PINNED
    public = rng.integers(0, 256, (states, 16)).astype(np.uint8)   # random public nibbles
    state = m ^ public                                              # the "keystream" whose XOR with public is m
    if gain_kind == "state":
        gain = rng.choice([-1.0, 1.0], (states, 1)) * rng.uniform(0.5, 2.0, (states, 1)) * 256.0 ** -w
        offset = rng.uniform(-3.0, 3.0, (states, 1))
    else:
        gain = rng.choice([-1.0, 1.0], nw) * rng.uniform(0.5, 2.0, nw)
        offset = rng.uniform(-3.0, 3.0, nw)
    one = states == 1
    spec = enc.value_slots((dtype, gain, offset))
    assert spec.groups == w and spec.distance == (0 if w == 1 else enc.stride * (4 if order == "transposed" else 1))
    lut = TypedValueLUT(ctx, spec)
    hi, lo = enc._pack(enc._order(state) >> 4), enc._pack(enc._order(state) & 0x0F)
    out = lut.apply_public(hi, lo, *enc.nibble_slots(public[0] if one else public))
    want = np.broadcast_to(gain, (states, nw)) * _want(m, dtype) + np.broadcast_to(offset, (states, nw))
    got = enc.values_from_slots(out, dtype)
    assert got.shape == ((nw,) if one else (states, nw))
    assert np.abs(got - (want[0] if one else want)).max() < 1e-9
    # every other slot -- the second byte's slot of each word and the slots that hold no state -- is 0
    word = np.zeros((states, 16))
    word[:, ::w] = 1.0
    rest = enc._float_slots(word) == 0.0
    assert rest.sum() == SC - (SC // enc.layout.period if periodic else 1) * states * nw
    assert not rest.any() or np.abs(out[rest]).max() < 1e-9  # periodic bytes fill every slot: nothing else to check
    assert np.abs(out.imag).max() < 1e-9
    assert [n for kind, n in ctx.calls if kind == "conj"] == [1]      # still one conjugation
    assert sum(n for kind, n in ctx.calls if kind == "rot") == (2 if w == 2 else 0)
    if batched:
        assert [n for kind, n in ctx.calls if kind == "mul"] == [2, 4, 8]  # depth unchanged: XOR_VALUE_DEPTH
    return enc, out, got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("states,periodic", [(1, False), (4, True), (4, False)])
@pytest.mark.parametrize("order", ["plain", "transposed"])
def test_typed_fallback(dtype, states, periodic, order):
    for k, kind in enumerate(("state", "word")):
        _run(dtype, states, order, periodic, kind, seed=100 * states + k)


def test_typed_fallback_unbatched():
    _run("<i2", 4, "plain", True, "word", seed=7, batched=False)


def test_pinned_values_read_as_expected():
    """the pinned block spelled out, so a wrong sign or byte order cannot hide behind a symmetric model"""
    assert _want(PINNED[None], "i1")[0, :4].tolist() == [-128.0, 0.0, 127.0, -1.0]
    assert _want(PINNED[None], "<i2")[0].tolist() == [128.0, -129.0, -256.0, 255.0, -32768.0, 32767.0, 32640.0, -1.0]
    assert _want(PINNED[None], ">u2")[0].tolist() == [32768.0, 32767.0, 255.0, 65280.0, 128.0, 65407.0, 32895.0, 65535.0]


def test_defaults_match_xor_value_lut():
    """u1 with the default gain and no offset: the typed spec gives the same slots as today's XorValueLUT"""
    from state_encoder import StateEncoder
    from xor_value_lut import TypedValueLUT, XorValueLUT
    ctx = RotCtx(SC)
    enc = StateEncoder(ctx, 4, periodic=True)
    rng = np.random.default_rng(5)
    st, pub = (rng.integers(0, 256, (4, 16)).astype(np.uint8) for _ in range(2))
    hi, lo = enc._pack(st >> 4), enc._pack(st & 0x0F)
    nib = enc.nibble_slots(pub)
    ref = XorValueLUT(ctx).apply_public(hi, lo, *nib)
    got = TypedValueLUT(ctx, enc.value_slots(("u1", None, 0.0))).apply_public(hi, lo, *nib)
    assert np.abs(got - ref).max() < 1e-9
    assert np.array_equal(np.rint(enc.values_from_slots(got) * 256.0).astype(np.uint8), st ^ pub)


class _Pipe:
    """AESPipeline's value methods on a numpy context: the keystream is a given pair"""

    def __init__(self, enc, pairs=1):
        from pipeline import AESPipeline
        self.ctx, self.encoder, self.layout, self.pairs = enc.ctx, enc, enc.layout, pairs
        self._value_luts = None
        for name in ("_no_pairs", "_typed_lut", "_value_lut", "to_values"):
            setattr(self, name, getattr(AESPipeline, name).__get__(self))


def test_pipeline_arguments():
    from state_encoder import StateEncoder
    ctx = RotCtx(SC)
    enc = StateEncoder(ctx, 4, periodic=True)
    pipe = _Pipe(enc)
    st = np.random.default_rng(6).integers(0, 256, (4, 16)).astype(np.uint8)
    hi, lo = enc._pack(st >> 4), enc._pack(st & 0x0F)
    assert pipe._typed_lut("u1", None, 0.0) is None and pipe._typed_lut("u1", 0.5, 0.0) is None  # today's path
    assert pipe._typed_lut("u1", None, 1.0) is not None and pipe._typed_lut("i1", None, 0.0) is not None
    out = pipe.to_values(hi, lo, dtype=">i2", gain=np.arange(1.0, 9.0), offset=0.25)
    assert np.abs(enc.values_from_slots(out, ">i2") - (np.arange(1.0, 9.0) * _want(st, ">i2") + 0.25)).max() < 1e-9
    out = pipe.to_values(hi, lo, dtype="<u2")  # the default gain is 256^-w: in [0, 1)
    assert np.abs(enc.values_from_slots(out, "<u2") - _want(st, "<u2") / 65536.0).max() < 1e-9
    with pytest.raises(ValueError, match="no precision"):
        pipe.to_values(hi, lo, dtype="<u4")
    with pytest.raises(ValueError):
        pipe.to_values(hi, lo, dtype="<i2", gain=np.ones(16))      # 8 words per state, not 16
    with pytest.raises(ValueError):
        pipe.to_values(hi, lo, dtype="i1", gain=np.ones((3, 16)))  # 4 states, not 3
    with pytest.raises(ValueError):
        pipe.to_values(hi, lo, dtype="i1", gain=np.inf)
    with pytest.raises(ValueError):
        _Pipe(enc, pairs=2).to_values(hi, lo, dtype="i1")


def test_decode_values_dtype_tag():
    from state_encoder import StateEncoder, tag_value_dtype

    class Ct:
        def __init__(self, slots):
            self.slots = slots

    ctx = RotCtx(SC)
    enc = StateEncoder(ctx, 1)
    st = np.arange(16, dtype=np.uint8) * 9
    out = np.zeros(SC)
    out[::2 * enc.stride][:8] = _want(st[None], "<i2")[0]
    ct = tag_value_dtype("<i2", Ct(out))
    assert np.array_equal(enc.decode_values(ct), _want(st[None], "<i2")[0])          # the tag is the default
    assert np.array_equal(enc.decode_values(ct, "<i2"), _want(st[None], "<i2")[0])
    with pytest.raises(ValueError, match="holds"):
        enc.decode_values(ct, ">i2")
    assert enc.decode_values(Ct(out)).shape == (16,)                                  # untagged: bytes, as before
    with pytest.raises(ValueError):
        enc.values_from_slots(out, "<u4")
