"""Public XOR fused with the value decode, on the host: coeffgen.xor_value_table,
xor_value_lut.XorValueLUT's fallback on the numpy slot context of test_public_xor (existing calls only), and
StateEncoder.values_from_slots against _pack."""
import numpy as np
import pytest

from test_public_xor import A_ALL, B_ALL, SlotCtx
from utils import ZetaEncoder


def test_xor_value_table():
    from coeffgen import xor_value_table
    E = xor_value_table()
    assert E.shape == (16, 16)
    a = ZetaEncoder.to_zeta(A_ALL, 16)
    full = sum(E[p, B_ALL] * a ** p for p in range(16))
    assert np.abs(full - (A_ALL ^ B_ALL)).max() < 1e-9          # all 256 (a, b) pairs
    assert np.abs(E[0] - 7.5).max() < 1e-12
    assert np.all(E[8].imag == 0.0)
    assert np.abs(E[8]).max() == pytest.approx(0.5, abs=1e-12)
    for p in range(1, 16):
        assert np.abs(E[16 - p] - np.conj(E[p])).max() < 1e-12  # the value is real
    assert np.abs(E).min() > 0.4                                # no entry is zero
    assert np.abs(E[1:]).max() == pytest.approx(np.abs(E[1]).max()) == pytest.approx(1.0 / (2.0 * np.sin(np.pi / 16)))
    T = sum(E[p, B_ALL] * a ** p for p in range(1, 8))
    real_form = 7.5 + E[8, B_ALL] * a ** 8 + T + np.conj(T)
    assert np.abs(real_form - (A_ALL ^ B_ALL)).max() < 1e-9
    assert np.abs(real_form.imag).max() < 1e-9


def test_xor_value_depth_constant():
    from utils import PUBLIC_XOR_DEPTH, XOR_VALUE_DEPTH
    assert XOR_VALUE_DEPTH == PUBLIC_XOR_DEPTH == 4


@pytest.mark.parametrize("batched", [True, False])
def test_apply_public_fallback_all_pairs(batched):
    from xor_value_lut import XorValueLUT
    gain = 1.0 / 256.0
    ctx = SlotCtx(256, batched)
    lut = XorValueLUT(ctx, gain)
    ah, al, bh, bl = A_ALL, A_ALL[::-1].copy(), B_ALL, np.roll(B_ALL, 37)  # all 256 pairs on both halves
    hi, lo = ZetaEncoder.to_zeta(ah, 16), ZetaEncoder.to_zeta(al, 16)
    out = lut.apply_public(hi, lo, bh.astype(np.uint8), bl.astype(np.uint8))
    assert np.abs(out - gain * (16 * (ah ^ bh) + (al ^ bl))).max() < 1e-9
    assert [n for kind, n in ctx.calls if kind == "conj"] == [1]  # exactly one conjugation
    muls = [n for kind, n in ctx.calls if kind == "mul"]
    # batched: the ct x ct products go through multiply_many, both nibbles' chains per depth (x^2 | x^3, x^4 | x^5..x^8)
    assert muls == ([2, 4, 8] if batched else [])
    ctx.calls.clear()
    plain = lut.apply(hi, lo)
    assert np.abs(plain - gain * (16 * ah + al)).max() < 1e-9
    assert [n for kind, n in ctx.calls if kind == "conj"] == [1]
    with pytest.raises(ValueError):
        lut.apply_public(hi, lo, np.full(256, 16, np.uint8), bl.astype(np.uint8))
    with pytest.raises(ValueError):
        lut.apply_public(hi, lo, bh.astype(np.uint8), bl[:255].astype(np.uint8))


def test_empty_slots_decode_to_zero():
    from xor_value_lut import XorValueLUT
    ctx = SlotCtx(64)
    out = XorValueLUT(ctx, 1.0).apply(np.ones(64, np.complex128), np.ones(64, np.complex128))
    assert np.abs(out).max() < 1e-9  # value 1 = zeta^0 on both halves: byte 0


@pytest.mark.parametrize("periodic,states,order", [(False, 1, "plain"), (False, 3, "plain"), (True, 4, "plain"),
                                                   (False, 3, "transposed"), (True, 4, "transposed")])
def test_values_from_slots_inverts_pack(periodic, states, order):
    from state_encoder import StateEncoder
    enc = StateEncoder(SlotCtx(512), states, periodic=periodic, byte_order=order)
    st = np.random.default_rng(states).integers(0, 256, (states, 16)).astype(np.uint8)
    arg = st[0] if states == 1 else st
    # the slot vector a value ciphertext decrypts to: byte / 256 where _pack puts the byte's nibbles, 0 elsewhere
    hi, lo = enc.nibble_slots(arg)
    slots = (16.0 * hi + lo) / 256.0 + 1e-7j  # a stray imaginary part is dropped
    got = enc.values_from_slots(slots)
    assert got.shape == arg.shape and got.dtype == np.float64
    assert np.array_equal(np.rint(got * 256.0).astype(np.uint8), arg)
    # the same order _pack itself uses: the Zeta16 image of the unpacked hi nibbles is _take of the packed vector
    ordered = enc._order(st)
    assert np.array_equal(ZetaEncoder.from_zeta(enc._take(enc._pack(ordered >> 4)), 16), ordered >> 4)
    with pytest.raises(ValueError):
        enc.values_from_slots(slots[:-1])
