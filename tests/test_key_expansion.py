"""key_expansion.py without an engine: the slot plan of the homomorphic AES-128 key schedule against
aes_keyschedule.expand_aes128_key, the coverage of its masked sums, and EngineContext.rot_pt_affine's fallback."""
import numpy as np
import pytest

SLOTS = 256
A1_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")  # FIPS-197 Appendix A.1

LAYOUTS = [(1, False), (1, True), (4, True), (3, False)]
ORDERS = ["plain", "transposed"]


def _encoder(states, periodic, order):
    """a StateEncoder used for its clear-byte side only (nibble_slots, _take, _order): no engine behind it"""
    from state_encoder import StateEncoder

    class Ctx:
        class engine:
            slot_count = SLOTS

    return StateEncoder(Ctx(), states, periodic=periodic, byte_order=order)


def _bytes_of(enc, hi, lo):
    out = enc._order(((enc._take(hi) << 4) | enc._take(lo)).astype(np.uint8))
    return out[0] if enc.states == 1 else out


def _expand_by_plan(enc, keys):
    """ten schedule_step_slots iterations from the keys (one per state): the 11 decoded round keys"""
    from key_expansion import schedule_step_slots
    x = enc.nibble_slots(keys)
    out = [_bytes_of(enc, *x)]
    for r in range(1, 11):
        x = schedule_step_slots(x, r, enc.layout, enc.byte_order)
        out.append(_bytes_of(enc, *x))
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("states,periodic", LAYOUTS)
def test_plan_expands_the_a1_key_and_random_keys(states, periodic, order):
    from aes_keyschedule import expand_aes128_key
    enc = _encoder(states, periodic, order)
    rng = np.random.default_rng(0xA1)
    # batches of one key per state: the A.1 key first, then random keys (9 keys or more in all, 8 of them random)
    batches = rng.integers(0, 256, (9 if states == 1 else 3, states, 16)).astype(np.uint8)
    batches[0, 0] = np.frombuffer(A1_KEY, np.uint8)
    for i, batch in enumerate(batches):
        got = _expand_by_plan(enc, batch[0] if states == 1 else batch)
        got = [g[None, :] if states == 1 else g for g in got]
        for b in range(states):
            want = expand_aes128_key(batch[b])
            for r in range(11):
                assert np.array_equal(got[r][b], want[r]), (states, periodic, order, i, b, r)
        if i == 0:
            assert bytes(got[1][0][:4]).hex() == "a0fafe17"
            assert bytes(got[10][0]).hex() == "d014f9a8c9ee2589e13f0cc8b6630ca6"


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("states,periodic", LAYOUTS)
def test_every_slot_is_covered_exactly_once(states, periodic, order):
    """per masked sum: every slot that holds a state byte is under exactly one mask or under the fill, every slot
    that holds none is under the fill, and masks and fill are 0 / 1"""
    from key_expansion import SchedulePlan
    from state_encoder import SlotLayout
    lay = SlotLayout(SLOTS, states, periodic)
    plan = SchedulePlan(lay, order)
    used = plan.used() > 0.5
    assert used.sum() == (SLOTS if periodic else 16 * states)
    for name, s in plan.sums().items():
        cover = np.sum(s.masks, axis=0)
        fill = s.fill if s.fill is not None else np.zeros(SLOTS)
        for v in (*s.masks, fill):
            assert np.all((v == 0) | (v == 1)), name
        assert np.all(cover + fill == 1), name
        assert np.all(fill[~used] == 1), name
        assert len(set(s.steps)) == len(s.steps) and all(st % lay.unit == 0 for st in s.steps), name
        # the shifts vacate k words of every state; the broadcast covers every used slot
        vacated = {"shift1": 4, "shift2": 8, "broadcast": 0}[name]
        assert int(fill[used].sum()) == vacated * used.sum() // 16, name
    assert len(plan.shift[1].steps) == len(plan.shift[2].steps) == 1
    assert len(plan.broadcast.steps) == 4  # the 8 (row, word) offset classes mod 16 positions


def test_stage_byte_model_matches_the_slot_model():
    from aes_keyschedule import expand_aes128_key
    from key_expansion import schedule_step_bytes, schedule_step_slots
    enc = _encoder(2, True, "transposed")
    keys = np.random.default_rng(3).integers(0, 256, (2, 16)).astype(np.uint8)
    stages = {}
    schedule_step_slots(enc.nibble_slots(keys), 1, enc.layout, enc.byte_order, stages)
    want = schedule_step_bytes(keys, 1)
    for name in ("prefix", "sub", "rot", "out"):
        assert np.array_equal(_bytes_of(enc, *stages[name]), want[name]), name
    assert np.array_equal(want["out"][1], expand_aes128_key(keys[1])[1])
    with pytest.raises(ValueError):
        schedule_step_slots(enc.nibble_slots(keys), 11, enc.layout, enc.byte_order)


class _NumpyEngine:
    """slot vectors as ciphertexts and plaintexts; no rot_pt_affine, so EngineContext takes its fallback"""
    slot_count = SLOTS

    def __init__(self):
        self.calls = []

    def rot_pt_sum(self, ct, steps, pts_per_output):
        self.calls.append(("rot_pt_sum", len(steps), len(pts_per_output)))
        return [sum(p * np.roll(ct, s) for p, s in zip(pts, steps) if p is not None) for pts in pts_per_output]

    def add(self, a, b):
        self.calls.append(("add",))
        return a + b


class _Stub:
    def __init__(self):
        self.engine = _NumpyEngine()


@pytest.mark.parametrize("order", ORDERS)
def test_context_fallback_equals_the_model(order):
    """EngineContext.rot_pt_affine on an engine without the entry: rot_pt_sum, then the fill added -- on numpy slot
    vectors of codewords it must give the codewords of the plan's nibble model"""
    from engine_context import EngineContext
    from key_expansion import SchedulePlan
    from state_encoder import SlotLayout
    from utils import ZetaEncoder
    lay = SlotLayout(SLOTS, 3, False)
    plan = SchedulePlan(lay, order)
    nib = np.random.default_rng(9).integers(0, 16, SLOTS).astype(np.uint8)
    z = ZetaEncoder.to_zeta(nib, 16)
    for name, s in plan.sums().items():
        stub = _Stub()
        pts = [m.astype(np.complex128) for m in s.masks]
        (out,) = EngineContext.rot_pt_affine(stub, z, s.steps, [pts], [s.fill])
        assert stub.engine.calls == [("rot_pt_sum", len(s.steps), 1), ("add",)], name
        assert np.allclose(out, ZetaEncoder.to_zeta(s.apply_slots(nib), 16), atol=1e-12), name
        assert np.allclose(out, s.apply_values(z), atol=1e-12), name
    # no fill: the plain sum, nothing added; one fill per output is required
    stub = _Stub()
    s = plan.broadcast
    two = EngineContext.rot_pt_affine(stub, z, s.steps, [s.masks, s.masks], [None, s.fill])
    assert stub.engine.calls == [("rot_pt_sum", 4, 2), ("add",)]
    assert np.allclose(two[0] + s.fill, two[1])
    with pytest.raises(ValueError):
        EngineContext.rot_pt_affine(stub, z, s.steps, [s.masks], [])


def test_encrypted_round_keys_container():
    from key_expansion import EncryptedRoundKeys
    from state_encoder import SlotLayout, tag_layout

    class Ct:
        pass

    lay, other = SlotLayout(SLOTS, 1, True), SlotLayout(SLOTS, 1, True)
    other.byte_order = "transposed"
    pairs = [(Ct(), Ct()) for _ in range(11)]
    erk = EncryptedRoundKeys.from_pairs(pairs, lay)
    assert len(erk) == 11 and erk[3] == pairs[3] and erk.packed == [None] * 11 and erk.key_basis == {}
    assert all(c.layout is lay for p in pairs for c in p)
    with pytest.raises(ValueError):
        EncryptedRoundKeys.from_pairs(pairs[:10], lay)
    tag_layout(other, *pairs[5])
    with pytest.raises(ValueError, match="transposed"):
        EncryptedRoundKeys.from_pairs(pairs, lay)
