"""XOR4 with a PUBLIC operand and the counter-mode byte helpers, on the host:
xor4_lut.public_tables, XOR4LUT.apply_public / apply_public_pair on a numpy slot context (the fallback
from existing calls only), StateEncoder.nibble_slots against _pack, ctr_mode.counter_blocks / ctr_xor."""
import numpy as np
import pytest

from utils import ZetaEncoder


@pytest.fixture(scope="module")
def xor4(coeff_dir):
    from add_round_key import load_xor4_coeffs
    return load_xor4_coeffs(coeff_dir / "xor4_coeffs.json")


class _Eng:
    def __init__(self, sc):
        self.slot_count = sc


class SlotCtx:
    """ciphertext = numpy slot vector, plaintext = numpy vector; records the batched calls"""

    def __init__(self, sc: int, batched: bool = True):
        self.engine = _Eng(sc)
        self.calls = []
        if batched:
            self.multiply_many = self._mm
            self.conjugate_many = self._cm

    def encode(self, v):
        return np.asarray(v, np.complex128)

    def multiply(self, a, b):
        return a * b

    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def add_plain(self, a, v):
        return a + v

    def conjugate(self, a):
        self.calls.append(("conj", 1))
        return np.conj(a)

    def _mm(self, pairs):
        self.calls.append(("mul", len(pairs)))
        return [a * b for a, b in pairs]

    def _cm(self, cts):
        self.calls.append(("conj", len(cts)))
        return [np.conj(c) for c in cts]


A_ALL, B_ALL = (g.reshape(-1) for g in np.meshgrid(np.arange(16), np.arange(16), indexing="ij"))
WANT = 256.0 * ZetaEncoder.to_zeta(A_ALL ^ B_ALL, 16)


def test_public_tables(xor4):
    from xor4_lut import public_tables
    T = public_tables(xor4)
    a = ZetaEncoder.to_zeta(A_ALL, 16)
    std = {p: a ** p if p <= 8 else np.conj(a ** (16 - p)) for p in range(16)}
    direct = sum(T.D[p, B_ALL] * std[p] for p in range(16))
    assert np.abs(direct - WANT).max() < 1e-9
    s1 = sum(T.d1[p, B_ALL] * a ** p for p in range(9))
    s2 = sum(T.d2[p, B_ALL] * a ** p for p in range(9))
    assert np.abs(s1 + np.conj(s2) - WANT).max() < 1e-9
    assert {p for p in range(16) if not np.any(T.D[p])} == set(range(0, 16, 2))  # exactly the even rows vanish
    assert T.need == {1, 3, 5, 7}  # a, a^3, a^5, a^7: depth 3
    assert np.abs(T.D).max() == pytest.approx(256.0, abs=1e-9)
    assert T.c1.shape == T.c2.shape == (9, 16)


@pytest.mark.parametrize("batched", [True, False])
def test_apply_public_fallback_all_pairs(xor4, batched):
    from xor4_lut import XOR4LUT
    ctx = SlotCtx(256, batched)
    x = XOR4LUT(ctx, xor4)
    out = x.apply_public(ZetaEncoder.to_zeta(A_ALL, 16), B_ALL.astype(np.uint8))
    assert np.abs(out - WANT).max() < 1e-9
    with pytest.raises(ValueError):
        x.apply_public(ZetaEncoder.to_zeta(A_ALL, 16), np.full(256, 16, np.uint8))
    with pytest.raises(ValueError):
        x.apply_public(ZetaEncoder.to_zeta(A_ALL, 16), B_ALL[:255].astype(np.uint8))


def test_apply_public_pair_batches_both_chains(xor4):
    from xor4_lut import XOR4LUT, _chain, _depth
    ctx = SlotCtx(256, True)
    x = XOR4LUT(ctx, xor4)
    rev = B_ALL[::-1].copy()
    o0, o1 = x.apply_public_pair(ZetaEncoder.to_zeta(A_ALL, 16), B_ALL.astype(np.uint8),
                                 ZetaEncoder.to_zeta(A_ALL, 16), rev.astype(np.uint8))
    assert np.abs(o0 - WANT).max() < 1e-9
    assert np.abs(o1 - 256.0 * ZetaEncoder.to_zeta(A_ALL ^ rev, 16)).max() < 1e-9
    muls = [n for kind, n in ctx.calls if kind == "mul"]
    depths = {_depth(k) for k, _, _ in _chain({1, 3, 5, 7})}
    assert len(muls) == len(depths) == 3  # one multiply_many per depth for both inputs' chains
    assert [n for kind, n in ctx.calls if kind == "conj"] == [2]  # both inputs conjugated in one batch


@pytest.mark.parametrize("periodic,states", [(False, 1), (False, 3), (True, 1), (True, 4)])
def test_nibble_slots_match_pack(periodic, states):
    from state_encoder import StateEncoder
    enc = StateEncoder(SlotCtx(512), states, periodic=periodic)
    st = np.random.default_rng(states).integers(0, 256, (states, 16)).astype(np.uint8)
    arg = st[0] if states == 1 else st
    hi, lo = enc.nibble_slots(arg)
    for nib, half in ((hi, st >> 4), (lo, st & 0x0F)):
        assert nib.dtype == np.uint8 and nib.shape == (512,) and nib.flags["C_CONTIGUOUS"]
        assert np.array_equal(ZetaEncoder.to_zeta(nib, 16), enc._pack(half))
    if not periodic:
        assert hi[states] == 0 and lo[states] == 0  # a slot that holds no state: nibble 0 (= the 1 _pack fills in)


def test_nibble_slots_refuses_pairs():
    from state_encoder import StateEncoder
    ctx = SlotCtx(512)
    ctx.stack = lambda cts: cts
    with pytest.raises(ValueError):
        StateEncoder(ctx, 1, pairs=2).nibble_slots(np.zeros(16, np.uint8))


def test_counter_blocks_layout_and_wrap():
    from ctr_mode import counter_blocks
    nonce = bytes(range(100, 112))
    b = counter_blocks(nonce, 0x01020304, 3)
    assert b.shape == (3, 16) and b.dtype == np.uint8
    assert all(bytes(r[:12]) == nonce for r in b)
    assert [bytes(r[12:]) for r in b] == [bytes([1, 2, 3, 4]), bytes([1, 2, 3, 5]), bytes([1, 2, 3, 6])]
    w = counter_blocks(nonce, 2 ** 32 - 1, 3)
    assert [bytes(r[12:]) for r in w] == [b"\xff\xff\xff\xff", b"\x00\x00\x00\x00", b"\x00\x00\x00\x01"]
    assert all(bytes(r[:12]) == nonce for r in w)  # the wrap never carries into the nonce
    assert counter_blocks(np.frombuffer(nonce, np.uint8), 7, 0).shape == (0, 16)
    with pytest.raises(ValueError):
        counter_blocks(nonce[:11], 0, 1)
    with pytest.raises(ValueError):
        counter_blocks(nonce, 2 ** 32, 1)


def test_ctr_xor_is_an_involution():
    from ctr_mode import counter_blocks, ctr_xor
    from oracle import aes_plain
    rng = np.random.default_rng(9)
    rks = aes_plain.expand_key(rng.integers(0, 256, 16).astype(np.uint8))
    fn = lambda blk: aes_plain.ref_encrypt(blk, rks)  # noqa: E731
    m = rng.integers(0, 256, (5, 16)).astype(np.uint8)
    nonce = rng.integers(0, 256, 12).astype(np.uint8)
    c = ctr_xor(fn, m, nonce, 2 ** 32 - 2)
    assert not np.array_equal(c, m)
    assert np.array_equal(ctr_xor(fn, c, nonce, 2 ** 32 - 2), m)
    assert np.array_equal(c[3] ^ m[3], fn(counter_blocks(nonce, 1, 1)[0]))  # block 3 of counter 2^32 - 2 uses counter 1
