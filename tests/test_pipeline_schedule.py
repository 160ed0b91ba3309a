"""AESPipeline's orchestration without an engine: the one key-schedule object behind the round keys
(key_expansion.ClearRoundKeys / EncryptedRoundKeys) and the order in which every transcipher_* and
to_* method refuses its arguments -- all of them before any keystream is computed.

The stand-ins bind the pipeline's own methods to an object whose encoder and XOR4 only count their calls, in the style
of tests/test_aes_key_sizes.py."""
import numpy as np
import pytest

SLOTS = 256
NONCE = bytes(12)


class _Ct:
    """a ciphertext: anything that takes a layout tag"""


class _CountingEncoder:
    def __init__(self):
        self.calls = []

    def _made(self, kind, *what):
        self.calls.append((kind, *what))
        return _Ct()

    def encode(self, key, seeded=False):
        return self._made("encode", bytes(key)), _Ct()

    def encode_packed(self, key):
        return self._made("encode_packed", bytes(key))

    def renorm_pack(self, hi, lo, level=None):
        return self._made("renorm_pack", hi, lo)

    def pack(self, hi, lo):
        return self._made("pack", hi, lo)

    def count(self, kind):
        return sum(c[0] == kind for c in self.calls)


class _CountingXor4:
    def __init__(self):
        self.calls = []

    def apply(self, x, key, out_level=None, keep_b=None, defer_conj=False):
        self.calls.append((key, keep_b, defer_conj))
        return _Ct()


class _SchedulePipe:
    """the pipeline's key-schedule methods on counting stand-ins (secret-key renorm mode, one state)"""

    def __init__(self, layout):
        from pipeline import AESPipeline
        self.encoder, self.xor4, self.layout = _CountingEncoder(), _CountingXor4(), layout
        self.states = self.pairs = 1
        self.fuse_sub_ark = self.true_fhe = False
        self.use_hard_renorm_between_steps = True
        self._schedule = None
        for name in ("_prepare_round_keys", "_check_encrypted_keys", "_encode_key", "_packed_round_key", "_fused_key",
                     "_ark_packed", "_floor"):
            setattr(self, name, getattr(AESPipeline, name).__get__(self))


def _layout():
    from state_encoder import SlotLayout
    return SlotLayout(SLOTS, 1, True)


def _keys(n, seed):
    return [k for k in np.random.default_rng(seed).integers(0, 256, (n, 16)).astype(np.uint8)]


def test_same_clear_schedule_twice_is_made_once():
    pipe = _SchedulePipe(_layout())
    keys = _keys(11, 1)
    rk = pipe._prepare_round_keys(keys)
    assert len(rk) == 11 and [c[1] for c in pipe.encoder.calls] == [bytes(k) for k in keys]  # each key once, in order
    assert pipe.encoder.count("encode_packed") == 0                                          # packed on first use only
    packed = [pipe._packed_round_key(r) for r in (1, 2, 1)]
    assert packed[0] is packed[2] and packed[0] is not packed[1]
    assert [c for c in pipe.encoder.calls if c[0] == "encode_packed"] == [("encode_packed", bytes(keys[1])), ("encode_packed", bytes(keys[2]))]
    fused = [pipe._fused_key(r, d) for r, d in ((10, +1), (10, -1), (10, +1))]
    assert fused[0] is fused[2] and fused[0] is not fused[1]
    pipe._ark_packed(_Ct(), 1)
    n_calls = len(pipe.encoder.calls)
    assert n_calls == 11 + 2 + 2
    # the same schedule again (equal bytes in new arrays): nothing is encoded, every entry is the one made before
    again = pipe._prepare_round_keys([k.copy() for k in keys])
    assert all(a is b for p, q in zip(again, rk) for a, b in zip(p, q))
    assert pipe._packed_round_key(1) is packed[0] and pipe._packed_round_key(2) is packed[1]
    assert pipe._fused_key(10, +1) is fused[0] and pipe._fused_key(10, -1) is fused[1]
    pipe._ark_packed(_Ct(), 1, defer_conj=True)
    assert len(pipe.encoder.calls) == n_calls
    (key_a, kb_a, defer_a), (key_b, kb_b, defer_b) = pipe.xor4.calls
    assert key_a is key_b is packed[0] and kb_a is kb_b and isinstance(kb_a, dict)  # one XOR4 basis dict per round
    assert defer_a is False and defer_b is False                                    # strict default: no conjugate fold


def test_another_schedule_rebuilds_everything():
    """15 keys, then 11, then the 15 again: the most recent clear schedule only, so each turn is made anew and nothing
    made for the previous schedule comes back"""
    pipe = _SchedulePipe(_layout())
    k15, k11 = _keys(15, 2), _keys(11, 3)
    k11[:] = k15[:11]  # the same leading bytes: only the count tells the schedules apart
    seen, encodes = [], 0
    for keys in (k15, k11, k15):
        rk = pipe._prepare_round_keys(keys)
        encodes += len(keys)
        assert len(rk) == len(keys) and pipe.encoder.count("encode") == encodes
        made = [c for p in rk for c in p] + [pipe._packed_round_key(1), *pipe._fused_key(len(keys) - 1, +1)]
        encodes += 1  # the fused key's
        pipe._ark_packed(_Ct(), 1)
        made.append(pipe.xor4.calls[-1][1])
        assert not any(m is old for m in made for old in seen)
        seen += made
        assert len(pipe._schedule.packed) == len(keys)
    assert pipe.encoder.count("encode_packed") == 3 and pipe.encoder.count("encode") == 15 + 11 + 15 + 3
    # other bytes at the same length are another schedule too
    other = [k.copy() for k in k15]
    other[14][15] ^= 1
    pipe._prepare_round_keys(other)
    assert pipe.encoder.count("encode") == 15 + 11 + 15 + 3 + 15 and pipe._schedule.packed == [None] * 15


def test_encrypted_round_keys_keep_their_caches_on_the_object():
    from key_expansion import EncryptedRoundKeys
    lay = _layout()
    pipe = _SchedulePipe(lay)
    erk = EncryptedRoundKeys.from_pairs([(_Ct(), _Ct()) for _ in range(13)], lay)
    assert pipe._prepare_round_keys(erk) is erk.pairs and pipe._schedule is erk
    p1 = pipe._packed_round_key(1)
    pipe._ark_packed(_Ct(), 1)
    assert erk.packed[1] is p1 and erk.packed[2] is None and set(erk.key_basis) == {1}
    assert pipe.xor4.calls[-1][:2] == (p1, erk.key_basis[1])
    assert pipe.encoder.calls == [("renorm_pack", *erk.pairs[1])]  # packed homomorphically: no key byte encoded
    # clear keys in between take the pipeline's schedule, not the object's caches
    pipe._prepare_round_keys(_keys(11, 4))
    assert pipe._packed_round_key(1) is not p1 and pipe._schedule is not erk
    n_calls = len(pipe.encoder.calls)
    assert pipe._prepare_round_keys(erk) is erk.pairs
    assert pipe._packed_round_key(1) is p1
    pipe._ark_packed(_Ct(), 1)
    assert pipe.xor4.calls[-1][:2] == (p1, erk.key_basis[1]) and len(pipe.encoder.calls) == n_calls
    # without the secret-key renorm the pack is the homomorphic one
    pipe.use_hard_renorm_between_steps = False
    assert erk.packed[2] is None and pipe._packed_round_key(2) is erk.packed[2]
    assert pipe.encoder.calls[-1] == ("pack", *erk.pairs[2])
    assert pipe.encoder.count("encode") == 11 and pipe.encoder.count("encode_packed") == 1  # the clear keys' only
    # refused before it becomes the schedule
    pipe.fuse_sub_ark = True
    other = EncryptedRoundKeys.from_pairs([(_Ct(), _Ct()) for _ in range(11)], lay)
    with pytest.raises(ValueError, match="fuse_sub_ark"):
        pipe._prepare_round_keys(other)
    assert pipe._schedule is erk


# ------------------------------------------------------------------ refusals come before the keystream
class _RefusalPipe:
    """every transcipher_* / to_* method and the LUT builders on a real StateEncoder's clear-byte side; the keystream
    and the engine are recorders that must never be reached"""

    BOUND = ("_no_pairs", "_typed_lut", "_value_lut", "_linear_lut", "_byte_lut", "_byte_bank", "_tag_bank",
             "transcipher_values", "transcipher_linear", "transcipher_lut", "transcipher_lut_bank",
             "to_values", "to_linear", "to_lut", "to_lut_bank")

    def __init__(self, pairs=1):
        from pipeline import AESPipeline
        from state_encoder import StateEncoder

        class Ctx:
            class engine:
                slot_count = SLOTS

        self.ctx = Ctx()
        self.encoder = StateEncoder(self.ctx, 2, periodic=True)
        self.layout, self.pairs, self.states = self.encoder.layout, pairs, 2
        self._value_luts = None
        self.keystreams = 0
        for name in self.BOUND:
            setattr(self, name, getattr(AESPipeline, name).__get__(self))

    def ctr_keystream(self, nonce12, counter0, round_keys):
        self.keystreams += 1
        raise AssertionError("the keystream was computed before the arguments were refused")


GOOD_CT = np.zeros((2, 16), np.uint8)
BAD_CT = np.zeros((3, 16), np.uint8)
GOOD_KEYS = [np.zeros(16, np.uint8)] * 13
BAD_KEYS = [np.zeros(16, np.uint8)] * 12
TABLE = np.arange(256.0)
# method suffix -> (good LUT arguments, bad ones, what the bad ones' ValueError says)
LUT_ARGS = {
    "values": ({}, {"dtype": "<u4"}, "value dtype"),
    "linear": ({"weight": np.eye(16)}, {"weight": np.eye(15)}, "W must be"),
    "lut": ({"table": TABLE}, {"table": TABLE[:255]}, "256 reals"),
    "lut_bank": ({"tables": TABLE[None], "select": [0]}, {"tables": TABLE[None, :255], "select": [0]}, "byte table bank"),
}


@pytest.mark.parametrize("kind", sorted(LUT_ARGS))
def test_transcipher_refusals_precede_the_keystream(kind):
    good, bad, says = LUT_ARGS[kind]
    pipe = _RefusalPipe()
    call = getattr(pipe, "transcipher_" + kind)
    # each refusal alone
    with pytest.raises(ValueError, match="11 round keys"):
        call(GOOD_CT, NONCE, 0, BAD_KEYS, **good)
    with pytest.raises(ValueError, match="uint8 state array"):
        call(BAD_CT, NONCE, 0, GOOD_KEYS, **good)
    with pytest.raises(ValueError, match=says):
        call(GOOD_CT, NONCE, 0, GOOD_KEYS, **bad)
    # and their order: pairs, key count, shape, the LUT's own arguments
    with pytest.raises(ValueError, match="multi-pair"):
        getattr(_RefusalPipe(pairs=2), "transcipher_" + kind)(BAD_CT, NONCE, 0, BAD_KEYS, **bad)
    with pytest.raises(ValueError, match="11 round keys"):
        call(BAD_CT, NONCE, 0, BAD_KEYS, **bad)
    with pytest.raises(ValueError, match="uint8 state array"):
        call(BAD_CT, NONCE, 0, GOOD_KEYS, **bad)
    assert pipe.keystreams == 0
    # with nothing to refuse the next step IS the keystream
    with pytest.raises(AssertionError, match="keystream"):
        call(GOOD_CT, NONCE, 0, GOOD_KEYS, **good)
    assert pipe.keystreams == 1


@pytest.mark.parametrize("kind", sorted(LUT_ARGS))
def test_conversion_refusals(kind):
    from state_encoder import SlotLayout, tag_layout
    _, bad, says = LUT_ARGS[kind]
    pipe = _RefusalPipe()
    call = getattr(pipe, "to_" + kind)
    ours = tag_layout(pipe.layout, _Ct(), _Ct())
    theirs = tag_layout(SlotLayout(SLOTS, 2, False), _Ct(), _Ct())
    with pytest.raises(ValueError, match="slot layout"):
        call(*theirs, **bad)  # the layout before the LUT's arguments
    with pytest.raises(ValueError, match=says):
        call(*ours, **bad)
    with pytest.raises(ValueError, match="multi-pair"):
        getattr(_RefusalPipe(pairs=2), "to_" + kind)(*theirs, **bad)
