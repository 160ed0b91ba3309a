"""A 16 x 16 linear map fused into the value decode, on the host: StateEncoder.linear_slots against
the float64 model W (q - zero_point) in_scale + bias, the dropped diagonals, and xor_value_lut.LinearValueLUT's
fallback loop (existing calls only) on the numpy slot context of test_value_typed."""
import numpy as np
import pytest

from test_value_typed import PINNED, SC, RotCtx, _Pipe

ORDERS = ["plain", "transposed"]
LAYOUTS = [(1, False), (4, True)]


def _bytes(st, dtype):
    """(states, 16) uint8 read as dtype, float64"""
    return np.ascontiguousarray(st).view(np.dtype(dtype)).astype(np.float64)


def _model(W, q, bias, in_scale, zp):
    """y[b, i] = sum_j W[b, i, j] (q[b, j] - zp[j]) in_scale + bias[b, i] in float64"""
    states = q.shape[0]
    Wb = np.broadcast_to(np.asarray(W, np.float64), (states, 16, 16))
    return np.einsum("bij,bj->bi", Wb, q - np.broadcast_to(zp, (16,))) * in_scale + np.broadcast_to(bias, (states, 16))


def _case(states, per_state, rng):
    W = rng.integers(-4, 5, (states, 16, 16) if per_state else (16, 16)).astype(np.float64)
    bias = rng.uniform(-2.0, 2.0, (states, 16))
    zp = rng.integers(-8, 9, 16).astype(np.float64)
    m = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    m[0] = PINNED
    return W, bias, zp, m


def _byte_slots(enc, st, dtype):
    """the slot vector holding each byte's number, read as dtype, in its slot (0 elsewhere)"""
    return enc._float_slots(_bytes(st, dtype))


@pytest.mark.parametrize("dtype", ["u1", "i1"])
@pytest.mark.parametrize("per_state", [False, True])
@pytest.mark.parametrize("states,periodic", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
def test_linear_slots_model(order, states, periodic, per_state, dtype):
    """sum_k roll(w_k * q_slots, steps_k) + affine equals the model to 1e-12; const is affine plus the groups' E_0 share"""
    from state_encoder import StateEncoder
    rng = np.random.default_rng(1000 * states + 10 * per_state + (dtype == "i1"))
    enc = StateEncoder(RotCtx(SC), states, periodic=periodic, byte_order=order)
    W, bias, zp, m = _case(states, per_state, rng)
    in_scale = 1.0 / 64.0
    spec = enc.linear_slots(W, bias, dtype, in_scale, zp)
    assert spec.weights.shape == spec.flags.shape == (spec.groups, SC) and spec.const.shape == (SC,)
    assert len(spec.steps) == spec.groups == len(spec.diagonals)
    assert spec.steps == [-k * enc.stride for k in spec.diagonals]
    state_slots = enc._float_slots(np.ones((states, 16))) != 0.0
    assert np.array_equal(spec.flags, np.tile((state_slots & (dtype == "i1")).astype(np.uint8), (spec.groups, 1)))
    q_slots = _byte_slots(enc, m, dtype)
    e0 = 16.0 * (-0.5 if dtype == "i1" else 7.5) + 7.5  # E_0 of both nibbles: the decode's R + T + conj(T) leaves it out
    got, share = spec.affine.copy(), np.zeros(SC)
    for w, st in zip(spec.weights, spec.steps):
        got += np.roll(w * q_slots, st)
        share += np.roll(w * e0, st)
    assert np.abs(spec.const - spec.affine - share).max() < 1e-12
    want = _model(W, _bytes(m, dtype), bias, in_scale, zp)
    assert np.abs(enc.values_from_slots(got).reshape(states, 16) - want).max() < 1e-12 * max(1.0, np.abs(want).max())
    assert not (~state_slots).any() or np.abs(got[~state_slots]).max() < 1e-12


@pytest.mark.parametrize("order", ORDERS)
def test_banded_matrix_three_groups(order):
    """a cyclic 3-tap filter in slot-position space: exactly the diagonals 0, 1 and 15 survive"""
    from state_encoder import StateEncoder
    enc = StateEncoder(RotCtx(SC), 4, periodic=True, byte_order=order)
    at = enc._order(np.arange(16, dtype=np.uint8)[None, :])[0].astype(int)
    Wp = np.zeros((16, 16))
    for po in range(16):
        Wp[po, po], Wp[po, (po + 1) % 16], Wp[po, (po - 1) % 16] = 2.0, -1.0, 0.5
    W = np.zeros((16, 16))
    W[np.ix_(at, at)] = Wp  # W'[po, pi] = W[at[po], at[pi]]
    spec = enc.linear_slots(W)
    assert spec.groups == 3 and spec.diagonals == [0, 1, 15]
    assert spec.steps == [0, -enc.stride, -15 * enc.stride]
    zero = enc.linear_slots(np.zeros((16, 16)), bias=1.5)  # nothing survives: one all-zero group keeps the op callable
    assert zero.groups == 1 and not zero.weights.any()


@pytest.mark.parametrize("order", ORDERS)
def test_diagonal_matrix_is_value_slots(order):
    from state_encoder import StateEncoder
    enc = StateEncoder(RotCtx(SC), 4, periodic=True, byte_order=order)
    d = np.random.default_rng(3).uniform(-2.0, 2.0, 16)
    in_scale = 1.0 / 128.0
    spec = enc.linear_slots(np.diag(d), 0.0, "i1", in_scale)
    ref = enc.value_slots(("i1", d * in_scale, 0.0))
    assert spec.groups == 1 and spec.steps == [0]
    assert np.array_equal(spec.weights, ref.weights) and np.array_equal(spec.flags, ref.flags)
    assert np.abs(spec.const - ref.const).max() < 1e-15


def _fallback(order, states, periodic, per_state, dtype, banded, seed, batched=True):
    from state_encoder import StateEncoder
    from xor_value_lut import LinearValueLUT
    rng = np.random.default_rng(seed)
    ctx = RotCtx(SC, batched)
    enc = StateEncoder(ctx, states, periodic=periodic, byte_order=order)
    W, bias, zp, m = _case(states, per_state, rng)
    if banded:
        i, j = np.indices((16, 16))
        at = enc._order(np.arange(16, dtype=np.uint8)[None, :])[0].astype(int)
        band = np.zeros((16, 16))
        band[np.ix_(at, at)] = np.isin((j - i) % 16, (0, 1, 2))  # three cyclic diagonals in slot-position space
        W = W * band
    public = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    state = m ^ public  # the "keystream" whose XOR with the public bytes is m
    lut = LinearValueLUT(ctx, enc.linear_slots(W, bias, dtype, None, zp))
    hi, lo = enc._pack(enc._order(state) >> 4), enc._pack(enc._order(state) & 0x0F)
    out = lut.apply_public(hi, lo, *enc.nibble_slots(public[0] if states == 1 else public))
    want = _model(W, _bytes(m, dtype), bias, 1.0 / 256.0, zp)
    got = enc.values_from_slots(out).reshape(states, 16)
    assert np.abs(got - want).max() < 1e-9
    rest = enc._float_slots(np.ones((states, 16))) == 0.0
    assert not rest.any() or np.abs(out[rest]).max() < 1e-9
    assert np.abs(out.imag).max() < 1e-9
    assert [n for kind, n in ctx.calls if kind == "conj"] == [1]  # one conjugation, the last key switch
    assert sum(n for kind, n in ctx.calls if kind == "rot") == 2 * sum(1 for st in lut.steps if st % SC)
    if batched:
        assert [n for kind, n in ctx.calls if kind == "mul"] == [2, 4, 8]  # depth unchanged: XOR_VALUE_DEPTH
    return lut


@pytest.mark.parametrize("dtype", ["u1", "i1"])
@pytest.mark.parametrize("states,periodic", LAYOUTS + [(4, False)])
@pytest.mark.parametrize("order", ORDERS)
def test_linear_fallback(order, states, periodic, dtype):
    lut = _fallback(order, states, periodic, True, dtype, False, seed=7 * states + (dtype == "i1"))
    assert lut.spec.groups == 16
    assert _fallback(order, states, periodic, False, dtype, True, seed=11 * states).spec.groups == 3


def test_linear_fallback_unbatched():
    _fallback("plain", 4, True, True, "i1", False, seed=5, batched=False)


def test_linear_value_errors():
    from state_encoder import LinearSlots, StateEncoder
    from xor_value_lut import LinearValueLUT
    ctx = RotCtx(SC)
    enc = StateEncoder(ctx, 4, periodic=True)
    W = np.eye(16)
    for dtype in ("<u2", ">u2", "<i2", ">i2"):
        with pytest.raises(ValueError):
            enc.linear_slots(W, dtype=dtype)
    with pytest.raises(ValueError, match="no precision"):
        enc.linear_slots(W, dtype="<u4")
    for bad in (np.eye(15), np.ones((3, 16, 16)), np.ones((16,)), np.ones((4, 16, 8))):
        with pytest.raises(ValueError, match="W must be"):
            enc.linear_slots(bad)
    with pytest.raises(ValueError):
        enc.linear_slots(W, bias=np.ones((3, 16)))
    with pytest.raises(ValueError):
        enc.linear_slots(W, zero_point=np.ones(8))
    with pytest.raises(ValueError, match="finite"):
        enc.linear_slots(np.full((16, 16), np.inf))

    class _Two:  # an encoder of two pairs without a stacking context: the refusal is linear_slots' own
        pairs = 2
    with pytest.raises(ValueError, match="pairs"):
        StateEncoder.linear_slots(_Two(), W)
    st = np.random.default_rng(6).integers(0, 256, (4, 16)).astype(np.uint8)
    hi, lo = enc._pack(st >> 4), enc._pack(st & 0x0F)
    pipe = _LinPipe(enc)
    out = pipe.to_linear(hi, lo, W, dtype="u1", in_scale=1.0)
    assert np.abs(enc.values_from_slots(out) - st).max() < 1e-9
    with pytest.raises(ValueError):
        pipe.to_linear(hi, lo, W, dtype="<i2")
    with pytest.raises(ValueError):
        _LinPipe(enc, pairs=2).to_linear(hi, lo, W)
    spec = enc.linear_slots(W)
    with pytest.raises(ValueError):
        LinearValueLUT(ctx, LinearSlots("i1", np.zeros((17, SC)), np.zeros((17, SC), np.uint8), spec.const, [0] * 17, list(range(17)), spec.affine))
    with pytest.raises(ValueError):
        LinearValueLUT(ctx, LinearSlots("i1", spec.weights, spec.flags, spec.const, [0, 1], [0], spec.affine))


class _LinPipe(_Pipe):
    """AESPipeline.to_linear on a numpy context"""

    def __init__(self, enc, pairs=1):
        from pipeline import AESPipeline
        super().__init__(enc, pairs)
        for name in ("_linear_lut", "to_linear"):
            setattr(self, name, getattr(AESPipeline, name).__get__(self))
