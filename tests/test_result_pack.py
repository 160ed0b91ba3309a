"""Result packs, the slot-level model and the client side (result_pack.py): numpy only, no GPU.

z = sum_j xi^(j k') * tile(m_j) and its inverse, the mean over all copies of a slot; the orthogonality the inverse rests
on; the sign convention against the monomial pair packing of DESIGN.md §4b (a rotation by one period negates X^k); the
meta through json; StateEncoder.decode_packed(array, meta) on model slots through stub contexts; the refusals.
"""
import json

import numpy as np
import pytest

SC = 4096  # N = 2^13: the largest case, G = 32 at period 64, needs 2048 slots


def _members(rng, count, period):
    return [rng.uniform(-1, 1, period) + 1j * rng.uniform(-1, 1, period) for _ in range(count)]


@pytest.mark.parametrize("period", [16, 64])
@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 8, 32])
def test_split_inverts_pack(count, period):
    from result_pack import group_size, pack_slots, split_slots
    rng = np.random.default_rng(100 * count + period)
    ms = _members(rng, count, period)
    G = group_size(count)
    assert G >= count and G < 2 * count and G & (G - 1) == 0
    z = pack_slots(ms, period, SC)
    assert z.shape == (SC,)
    got = split_slots(z, G, period)
    assert len(got) == G
    for j in range(G):
        want = np.tile(ms[j], SC // period) if j < count else np.zeros(SC)
        assert got[j].shape == (SC,)
        assert np.abs(got[j] - want).max() < 1e-12, (j, float(np.abs(got[j] - want).max()))
    # full-length members are taken slot by slot (what a decryption with noise on it needs)
    assert np.abs(pack_slots([np.tile(m, SC // period) for m in ms], period, SC) - z).max() < 1e-12


def test_absent_member_is_zero():
    from result_pack import pack_slots, split_slots
    rng = np.random.default_rng(7)
    ms = _members(rng, 5, 16)
    ms[1] = None
    ms[4] = None
    got = split_slots(pack_slots(ms, 16, SC), 8, 16)
    for j in range(8):
        want = np.zeros(SC) if j >= 5 or ms[j] is None else np.tile(ms[j], SC // 16)
        assert np.abs(got[j] - want).max() < 1e-12


@pytest.mark.parametrize("G,period", [(2, 16), (8, 16), (32, 64), (4, 1024)])
def test_columns_are_orthogonal(G, period):
    """for every slot t of one period the columns (xi_(t + period u)^(j k'))_u, j < G, are orthogonal of norm^2 sc / period"""
    from result_pack import pack_phases
    ph = pack_phases(G, period, SC).reshape(G, SC // period, period)
    for t in (0, 1, period // 2, period - 1):
        A = ph[:, :, t].T  # (copies, G)
        gram = A.conj().T @ A
        assert np.abs(gram - (SC // period) * np.eye(G)).max() < 1e-9


def test_split_projects_noise_with_norm_one():
    """each output slot is a mean of unit-modulus multiples of the pack's slots: whatever error sits on the pack, no
    member's largest slot error exceeds the pack's largest"""
    from result_pack import pack_slots, split_slots
    rng = np.random.default_rng(11)
    ms = _members(rng, 4, 16)
    z = pack_slots(ms, 16, SC)
    noise = 1e-3 * (rng.standard_normal(SC) + 1j * rng.standard_normal(SC))
    got = split_slots(z + noise, 4, 16)
    for j in range(4):
        assert np.abs(got[j] - np.tile(ms[j], SC // 16)).max() <= np.abs(noise).max()


def test_convention_is_the_monomial_pair_packing():
    """z = a + X^k b, k = N / 4 period, and the rotation by `period` slots (np.roll) fixes a and negates
    X^k b.  For four members, pack([a, c, b, d]) at `period` is the pair packing of (a, b) and (c, d) packed again at
    2 period"""
    from result_pack import pack_phases, pack_slots
    rng = np.random.default_rng(13)
    period = 16
    a, b, c, d = [np.tile(m, SC // period) for m in _members(rng, 4, period)]
    xk = pack_phases(2, period, SC)[1]            # the slot vector of X^(N / 4 period)
    z = pack_slots([a, b], period, SC)
    assert np.abs(z - (a + xk * b)).max() < 1e-12
    for r in (period, -period):
        assert np.abs(np.roll(z, r) - (a - xk * b)).max() < 1e-12
    x2 = pack_phases(2, 2 * period, SC)[1]        # X^(N / 8 period)
    quad = (a + xk * b) + x2 * (c + xk * d)
    assert np.abs(pack_slots([a, c, b, d], period, SC) - quad).max() < 1e-12


# ---------------------------------------------------------------- stub contexts: the wire without an engine
class _Ct:
    """a `ciphertext` of the stub server: its slot vector and the two tags"""

    def __init__(self, slots, layout=None, value_dtype=None):
        self.slots, self.layout = np.asarray(slots, np.complex128), layout
        if value_dtype is not None:
            self.value_dtype = value_dtype


class _Eng:
    def __init__(self, sc):
        self.slot_count = sc

    def export(self, ct):
        return ct.slots

    def import_ct(self, array, level):
        assert level == 0
        return _Ct(array)

    def check(self, ct):
        return None


class _Ctx:
    """pack_periodic is the slot model; export / import carry the slot vector itself; decrypt reads it"""

    def __init__(self, sc=SC):
        self.engine = _Eng(sc)
        self.packs = []

    def stack(self, cts):
        raise AssertionError("no stacks here")

    def pack_periodic(self, cts, period):
        from result_pack import group_size, pack_slots
        self.packs.append((len(cts), period))
        z = _Ct(pack_slots([None if c is None else c.slots for c in cts], period, self.engine.slot_count))
        z.pack = (group_size(len(cts)), period)
        return z

    def decrypt(self, ct):
        return ct.slots


def _tagged(enc, state, values, dtype="u1", gain=1.0 / 256.0):
    from state_encoder import tag_layout, tag_value_dtype
    st = enc._as_batch(state)
    hi, lo = tag_layout(enc.layout, _Ct(enc._pack(st >> 4)), _Ct(enc._pack(st & 0x0F)))
    val = tag_value_dtype(dtype, tag_layout(enc.layout, _Ct(enc._float_slots(gain * np.asarray(values, np.float64))))[0])
    return hi, lo, val


@pytest.mark.parametrize("byte_order", ["plain", "transposed"])
@pytest.mark.parametrize("states", [1, 4])
def test_decode_packed_on_model_slots(states, byte_order):
    from result_pack import dump_results
    from state_encoder import StateEncoder
    server, client = _Ctx(), _Ctx()
    enc = StateEncoder(server, states, periodic=True, byte_order=byte_order)
    rng = np.random.default_rng(17 + states)
    state = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    vals = rng.integers(0, 256, (states, 16)).astype(np.uint8)
    hi, lo, val = _tagged(enc, state if states > 1 else state[0], vals)
    array, meta = dump_results(server, [hi, lo, val])
    assert server.packs == [(3, 16 * states)]                      # the members' common layout period
    assert (meta["members"], meta["G"], meta["period"], meta["slots"]) == (3, 4, 16 * states, SC)
    assert meta["value_dtypes"] == [None, None, "u1"] and all(t["states"] == states and t["byte_order"] == byte_order for t in meta["layouts"])
    meta2 = json.loads(json.dumps(meta))                           # a plain dict: it survives the wire
    assert meta2 == meta
    cenc = StateEncoder(client, states, periodic=True, byte_order=byte_order)
    noise = 1e-3 * np.random.default_rng(5).standard_normal(SC)
    out = cenc.decode_packed(array + noise, meta2)
    assert len(out) == 2
    assert np.array_equal(out[0], state if states > 1 else state[0])
    want = vals if states > 1 else vals[0]
    assert out[1].shape == want.shape and np.array_equal(np.rint(256.0 * out[1]).astype(np.int64), want.astype(np.int64))
    # value first, then the pair; and decode_slots / values_from_slots on unpack_results' vectors give the same
    from result_pack import unpack_results
    array, meta = dump_results(server, [val, hi, lo])
    out = cenc.decode_packed(array, meta)
    assert np.array_equal(out[1], state if states > 1 else state[0]) and np.abs(256.0 * out[0] - want).max() < 1e-9
    sl = unpack_results(client, array, meta)
    assert len(sl) == 3 and all(s.shape == (SC,) for s in sl)
    assert np.array_equal(cenc.decode_slots(sl[1], sl[2]), out[1])
    assert np.array_equal(cenc.values_from_slots(sl[0], "u1"), out[0])


def test_mixed_periods_and_explicit_period():
    from result_pack import pack_results
    from state_encoder import StateEncoder
    ctx = _Ctx()
    e1, e4 = StateEncoder(ctx, 1, periodic=True), StateEncoder(ctx, 4, periodic=True)
    a = _tagged(e1, np.zeros(16, np.uint8), np.zeros(16))[0]
    b = _tagged(e4, np.zeros((4, 16), np.uint8), np.zeros((4, 16)))[0]
    assert pack_results(ctx, [a, b]).pack == (2, 64)               # the largest period; 16 divides it
    assert pack_results(ctx, [a, None, b], period=128).pack == (4, 128)
    plain = _Ct(np.zeros(SC))
    assert pack_results(ctx, [plain, a], period=32).pack == (2, 32)
    with pytest.raises(ValueError, match="explicit period"):
        pack_results(ctx, [plain, a])
    with pytest.raises(ValueError, match="does not divide"):
        pack_results(ctx, [a, b], period=32)


def test_value_errors():
    from result_pack import dump_results, pack_results, pack_slots, split_slots, unpack_results
    from state_encoder import StateEncoder
    server = _Ctx()
    enc = StateEncoder(server, 1, periodic=True)
    hi, lo, val = _tagged(enc, np.arange(16, dtype=np.uint8), np.arange(16))
    array, meta = dump_results(server, [hi, lo, val])
    # --- the encoder's refusals
    with pytest.raises(ValueError, match="pairs > 1"):
        StateEncoder(server, 1, periodic=True, pairs=2).decode_packed(array, meta)
    with pytest.raises(ValueError, match="reference layout"):
        StateEncoder(server, 1, periodic=False).decode_packed(array, meta)
    with pytest.raises(ValueError, match="slots"):
        StateEncoder(_Ctx(SC // 2), 1, periodic=True).decode_packed(array[:SC // 2], meta)
    with pytest.raises(ValueError, match="slot layout"):
        StateEncoder(server, 1, periodic=True, byte_order="transposed").decode_packed(array, meta)
    with pytest.raises(ValueError, match="period|slot layout"):
        StateEncoder(server, 4, periodic=True).decode_packed(array, meta)
    for members in ([hi, val], [hi, lo, lo, val], [val, hi]):
        arr, m = dump_results(server, members)
        with pytest.raises(ValueError, match="odd run"):
            enc.decode_packed(arr, m)
    arr, m = dump_results(server, [hi, None, lo])
    with pytest.raises(ValueError, match="absent"):
        enc.decode_packed(arr, m)
    with pytest.raises(ValueError):
        enc.decode_slots(np.zeros(SC // 2), np.zeros(SC))
    with pytest.raises(ValueError):
        StateEncoder(server, 1, periodic=True, pairs=2).decode_slots(np.zeros(SC), np.zeros(SC))
    assert np.array_equal(enc.decode_packed(array, meta)[0], np.arange(16, dtype=np.uint8))   # and the encoder still decodes
    # --- the module's
    with pytest.raises(ValueError, match="1..32"):
        pack_results(server, [hi] * 33)
    with pytest.raises(ValueError, match="1..32"):
        pack_results(server, [])
    with pytest.raises(ValueError, match="absent"):
        pack_results(server, [None, None], period=16)
    with pytest.raises(ValueError, match="non-periodic"):
        pack_results(server, [_tagged(StateEncoder(server, 1), np.zeros(16, np.uint8), np.zeros(16))[0]])   # the reference layout
    with pytest.raises(ValueError, match="power of two"):
        pack_slots([np.zeros(24)], 24, SC)
    with pytest.raises(ValueError, match="exceeds"):
        pack_slots([np.zeros(1024)] * 8, 1024, SC)
    with pytest.raises(ValueError, match="power of two"):
        split_slots(np.zeros(SC), 3, 16)
    with pytest.raises(ValueError):
        pack_slots([np.zeros(17)], 16, SC)
    bad = dict(meta, G=8)
    with pytest.raises(ValueError, match="does not belong"):
        unpack_results(server, array, bad)
    with pytest.raises(ValueError, match="slots"):
        unpack_results(_Ctx(SC // 2), array, meta)


def test_an_engine_without_the_entry_point_is_an_error():
    """the house pattern: a missing kernel is an error, never a quiet host fallback"""
    from result_pack import pack_results

    class Bare:
        class engine:
            slot_count = SC

    with pytest.raises(RuntimeError, match="aesfhe_pack_periodic"):
        pack_results(Bare(), [_Ct(np.zeros(SC))], period=16)
