"""A bank of byte tables with a table per slot and several outputs per call, on the host:
StateEncoder.lut_bank_slots' placement, xor_value_lut.ByteValueBank's fallback loop (existing calls only) on the numpy
slot context of test_value_typed, its identity with ByteValueLUT for one table, and the refusals."""
import numpy as np
import pytest

from test_byte_lut import LAYOUTS, ORDERS, TABLES, X, _LutPipe
from test_value_typed import SC, RotCtx

BANK = np.stack([TABLES["relu"], TABLES["mulaw"], TABLES["random"]])  # T = 3


def _enc(states, periodic, order, batched=True):
    from state_encoder import StateEncoder
    ctx = RotCtx(SC, batched)
    return ctx, StateEncoder(ctx, states, periodic=periodic, byte_order=order)


def _selectors(rng, states, T):
    """a per-byte selector (16,), a per-state-and-byte one (states, 16) and a scalar"""
    return [rng.integers(0, T, 16), rng.integers(0, T, (states, 16)), int(rng.integers(0, T))]


@pytest.mark.parametrize("states,periodic", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
def test_placement(states, periodic, order):
    """values_from_slots of the float copy of sel gives back select; slots without a state hold 0; the weights are
    lut_slots' and const is weights * c00s[sel]"""
    _, enc = _enc(states, periodic, order)
    rng = np.random.default_rng(10 * states + periodic)
    c00s = rng.uniform(-1.0, 1.0, 5)
    gain = rng.uniform(-2.0, 2.0, (states, 16))
    rest = enc._float_slots(np.ones((states, 16))) == 0.0
    for select in _selectors(rng, states, 5):
        sel, weights, const = enc.lut_bank_slots(select, gain, c00s)
        assert sel.dtype == np.uint8 and sel.shape == (SC,)
        back = enc.values_from_slots(sel.astype(np.float64), "lut").reshape(states, 16)
        assert np.array_equal(back, np.broadcast_to(select, (states, 16)))
        assert not sel[rest].any()
        assert np.array_equal(weights, enc.lut_slots(gain)[0])
        assert np.array_equal(const, weights * c00s[sel])


def _run(order, states, periodic, public, seed, batched=True):
    from utils import BYTE_LUT_DEPTH
    from xor_value_lut import ByteValueBank
    rng = np.random.default_rng(seed)
    ctx, enc = _enc(states, periodic, order, batched)
    T, K = len(BANK), 2
    m = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    m[0, :4] = (0x00, 0x7F, 0x80, 0xFF)
    pub = rng.integers(0, 256, (states, 16)).astype(np.uint8) if public else np.zeros((states, 16), np.uint8)
    state = m ^ pub
    selects = [rng.integers(0, T, (states, 16)), np.arange(16) % T]
    gains = [rng.uniform(-2.0, 2.0, (states, 16)), -1.5]
    c00s = BANK.mean(axis=1)
    bank = ByteValueBank(ctx, BANK, [enc.lut_bank_slots(s, g, c00s) for s, g in zip(selects, gains)])
    assert bank.DEPTH == BYTE_LUT_DEPTH == 5 and np.abs(bank.c00 - c00s).max() < 1e-15
    hi, lo = enc._pack(enc._order(state) >> 4), enc._pack(enc._order(state) & 0x0F)
    if public:
        outs = bank.apply_public(hi, lo, *enc.nibble_slots(pub[0] if states == 1 else pub))
    else:
        outs = bank.apply(hi, lo)
    assert len(outs) == K
    rest = enc._float_slots(np.ones((states, 16))) == 0.0
    for out, select, gain in zip(outs, selects, gains):
        got = enc.values_from_slots(out, "lut").reshape(states, 16)
        want = gain * BANK[np.broadcast_to(select, (states, 16)), m]
        assert np.abs(got - want).max() < 1e-9
        assert not rest.any() or np.abs(out[rest]).max() < 1e-9  # slots without a state: 0
        assert np.abs(out.imag).max() < 1e-9
    if batched:
        assert [n for kind, n in ctx.calls if kind == "mul"] == [2, 4, 8, 15 * K]  # the bases, then ONE batch for all outputs
        assert [n for kind, n in ctx.calls if kind == "conj"] == [7, K]            # conj(lo^1..7) once, then the K conj(T)


@pytest.mark.parametrize("public", [True, False], ids=["public", "zero"])
@pytest.mark.parametrize("states,periodic", LAYOUTS)
@pytest.mark.parametrize("order", ORDERS)
def test_bank_fallback(order, states, periodic, public):
    _run(order, states, periodic, public, seed=100 * states + 10 * public + periodic)


def test_bank_fallback_unbatched():
    _run("transposed", 4, True, True, seed=5, batched=False)


@pytest.mark.parametrize("name", ["mulaw", "random"])
def test_one_table_is_byte_value_lut(name):
    """T = 1, K = 1, select = 0: the same float operations in the same order as ByteValueLUT, so the same bits"""
    from coeffgen import byte_value_table
    from xor_value_lut import ByteValueBank, ByteValueLUT
    ctx, enc = _enc(4, True, "transposed")
    rng = np.random.default_rng(11)
    f = TABLES[name]
    st, pub = (rng.integers(0, 256, (4, 16)).astype(np.uint8) for _ in range(2))
    gain = rng.uniform(-2.0, 2.0, (4, 16))
    hi, lo = enc._pack(enc._order(st) >> 4), enc._pack(enc._order(st) & 0x0F)
    nib = enc.nibble_slots(pub)
    ref = ByteValueLUT(ctx, f, enc.lut_slots(gain)[0]).apply_public(hi, lo, *nib)
    calls = list(ctx.calls)
    del ctx.calls[:]
    got = ByteValueBank(ctx, f[None, :], [enc.lut_bank_slots(0, gain, [byte_value_table(f)[1]])]).apply_public(hi, lo, *nib)
    assert len(got) == 1 and np.array_equal(got[0], ref)
    assert ctx.calls == calls  # and the same batched calls


class _BankPipe(_LutPipe):
    """AESPipeline.to_lut_bank on a numpy context"""

    def __init__(self, enc, pairs=1):
        from pipeline import AESPipeline
        super().__init__(enc, pairs)
        for name in ("_byte_bank", "_tag_bank", "to_lut_bank"):
            setattr(self, name, getattr(AESPipeline, name).__get__(self))


def test_value_errors():
    from state_encoder import StateEncoder
    from xor_value_lut import ByteValueBank
    ctx, enc = _enc(4, True, "plain")
    c00s = BANK.mean(axis=1)
    # lut_bank_slots: a non-integer or out-of-range select, a shape that does not broadcast, pairs > 1
    for bad in (1.0, np.ones(16), np.ones(16, bool), -1, 3, np.full((4, 16), 3), np.zeros(15, int), np.zeros((3, 16), int), np.zeros((4, 8), int)):
        with pytest.raises(ValueError):
            enc.lut_bank_slots(bad, 1.0, c00s)
    with pytest.raises(ValueError):
        enc.lut_bank_slots(0, np.ones((3, 16)), c00s)
    with pytest.raises(ValueError):
        enc.lut_bank_slots(0, np.inf, c00s)

    class _Two:  # an encoder of two pairs without a stacking context: the refusal is lut_bank_slots' own
        pairs = 2
    with pytest.raises(ValueError, match="pairs"):
        StateEncoder.lut_bank_slots(_Two(), 0, 1.0, c00s)
    # ByteValueBank: tables (T, 256) finite with 1 <= T <= 64, K >= 1 outputs of per-slot vectors
    good = enc.lut_bank_slots(np.arange(16) % 3, 1.0, c00s)
    bad_tables = [BANK[0], BANK[:, :255], BANK[:0], np.tile(BANK[0], (65, 1)), np.where(X == 3, np.nan, BANK), np.where(X == 200, np.inf, BANK)]
    for bad in bad_tables:
        with pytest.raises(ValueError):
            ByteValueBank(ctx, bad, [good])
    with pytest.raises(ValueError):
        ByteValueBank(ctx, BANK, [])
    sel, w, c = good
    for bad in ((sel[:-1], w, c), (sel.astype(np.int64), w, c), (np.full(SC, 3, np.uint8), w, c), (sel, w[:-1], c),
                (sel, np.where(np.arange(SC) == 7, np.nan, w), c), (sel, w, c[:-1])):
        with pytest.raises(ValueError):
            ByteValueBank(ctx, BANK, [bad])
    bank = ByteValueBank(ctx, BANK, [good])
    st = np.random.default_rng(6).integers(0, 256, (4, 16)).astype(np.uint8)
    hi, lo = enc._pack(st >> 4), enc._pack(st & 0x0F)
    zero = np.zeros(SC, np.uint8)
    with pytest.raises(ValueError):
        bank.apply_public(hi, lo, np.full(SC, 16, np.uint8), zero)
    with pytest.raises(ValueError):
        bank.apply_public(hi, lo, zero[:-1], zero[:-1])
    # the pipeline: K selectors, one gain or K of them
    pipe = _BankPipe(enc)
    byte = np.arange(16) % 3
    outs = pipe.to_lut_bank(hi, lo, BANK, [byte, 1], gain=[np.arange(1.0, 17.0), -1.0])
    assert len(outs) == 2
    assert np.abs(enc.values_from_slots(outs[0], "lut") - np.arange(1.0, 17.0) * BANK[byte, st]).max() < 1e-9
    assert np.abs(enc.values_from_slots(outs[1], "lut") + BANK[1][st]).max() < 1e-9
    outs = pipe.to_lut_bank(hi, lo, BANK, [byte, 1, np.full((4, 16), 2)], gain=0.5)  # one gain for all outputs
    assert np.abs(enc.values_from_slots(outs[2], "lut") - 0.5 * BANK[2][st]).max() < 1e-9
    for bad in bad_tables:
        with pytest.raises(ValueError):
            pipe.to_lut_bank(hi, lo, bad, [0])
    for bad in ([], 0, [3], [np.zeros((3, 16), int)], [0.0]):
        with pytest.raises(ValueError):
            pipe.to_lut_bank(hi, lo, BANK, bad)
    for bad in ([1.0], [1.0, 2.0, 3.0], [np.ones((3, 16)), 1.0]):
        with pytest.raises(ValueError):
            pipe.to_lut_bank(hi, lo, BANK, [0, 1], gain=bad)
    with pytest.raises(ValueError):
        _BankPipe(enc, pairs=2).to_lut_bank(hi, lo, BANK, [0])
