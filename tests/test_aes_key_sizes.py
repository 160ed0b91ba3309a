"""AES-192 / AES-256 without an engine: the byte models against the published vectors of FIPS-197
Appendix C and NIST SP 800-38A Appendix F.5, the slot plan of the 256-bit key schedule against
aes_keyschedule.expand_aes_key, the word copy's masked sum, the 13- and 15-key containers and the refusals.

The vectors below were compared once, digit for digit, with the published documents (FIPS-197 C.1 - C.3, SP 800-38A
F.5.3 and F.5.5); where `cryptography` or `Crypto` is installed the block function is checked against it too."""
from types import SimpleNamespace

import numpy as np
import pytest

SLOTS = 256
PT = "00112233445566778899aabbccddeeff"
C1_CT = "69c4e0d86a7b0430d8cdb78070b4c55a"   # FIPS-197 C.1, key 00..0f
C2_CT = "dda97ca4864cdfe06eaf70a0ec0d7191"   # FIPS-197 C.2, key 00..17
C3_CT = "8ea2b7ca516745bfeafc49904b496089"   # FIPS-197 C.3, key 00..1f
F5_NONCE, F5_COUNTER0 = bytes(range(0xF0, 0xFC)), 0xFCFDFEFF   # SP 800-38A F.5: initial counter block f0f1...ff
F5_PT = ["6bc1bee22e409f96e93d7e117393172a", "ae2d8a571e03ac9c9eb76fac45af8e51"]
F55_KEY = "603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"
F55_CT = ["601ec313775789a5b7a7f504bbf3d228", "f443e3ca4d62b59aca84e990cacaf5c5"]
F53_KEY = "8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"
F53_CT0 = "1abc932417521ca24f2b0459fe7e6e0b"

LAYOUTS = [(1, False), (1, True), (3, False)]   # reference and periodic layout, states 1 and 3
ORDERS = ["plain", "transposed"]


def _hex(s):
    return np.frombuffer(bytes.fromhex(s), np.uint8)


def _encoder(states, periodic, order):
    """a StateEncoder used for its clear-byte side only (tests/test_key_expansion.py)"""
    from state_encoder import StateEncoder

    class Ctx:
        class engine:
            slot_count = SLOTS

    return StateEncoder(Ctx(), states, periodic=periodic, byte_order=order)


def _bytes_of(enc, hi, lo):
    out = enc._order(((enc._take(hi) << 4) | enc._take(lo)).astype(np.uint8))
    return out[0] if enc.states == 1 else out


# ------------------------------------------------------------------ published vectors
@pytest.mark.parametrize("nbytes,ct", [(16, C1_CT), (24, C2_CT), (32, C3_CT)])
def test_fips197_appendix_c(nbytes, ct):
    from aes_keyschedule import expand_aes_key
    from ctr_mode import fips_block_fn
    key = np.arange(nbytes, dtype=np.uint8)
    rks = expand_aes_key(key)
    assert len(rks) == nbytes // 4 + 7 and all(k.shape == (16,) and k.dtype == np.uint8 for k in rks)
    assert bytes(fips_block_fn(rks)(_hex(PT))).hex() == ct
    # FIPS-197 A.3 / C.3: the last words of the 256-bit schedule
    if nbytes == 32:
        assert bytes(rks[14]).hex() == "24fc79ccbf0979e9371ac23c6d68de36"
    for lib in ("cryptography", "Crypto"):
        try:
            if lib == "cryptography":
                from cryptography.hazmat.primitives.ciphers import Cipher, algorithms, modes
                enc = Cipher(algorithms.AES(bytes(key)), modes.ECB()).encryptor()
                got = enc.update(bytes.fromhex(PT)) + enc.finalize()
            else:
                from Crypto.Cipher import AES
                got = AES.new(bytes(key), AES.MODE_ECB).encrypt(bytes.fromhex(PT))
        except ImportError:
            continue
        assert got.hex() == ct, lib


def test_sp800_38a_ctr_aes256_and_aes192():
    from aes_keyschedule import expand_aes_key
    from ctr_mode import counter_blocks, ctr_xor, fips_block_fn
    assert bytes(counter_blocks(F5_NONCE, F5_COUNTER0, 1)[0]).hex() == "f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff"
    pt = np.stack([_hex(p) for p in F5_PT])
    got = ctr_xor(fips_block_fn(expand_aes_key(_hex(F55_KEY))), pt, F5_NONCE, F5_COUNTER0)
    assert [bytes(b).hex() for b in got] == F55_CT
    got = ctr_xor(fips_block_fn(expand_aes_key(_hex(F53_KEY))), pt[:1], F5_NONCE, F5_COUNTER0)
    assert bytes(got[0]).hex() == F53_CT0


def test_expand_aes_key_lengths():
    from aes_keyschedule import expand_aes128_key, expand_aes_key
    rng = np.random.default_rng(0x192)
    k = rng.integers(0, 256, 16).astype(np.uint8)
    assert all(np.array_equal(a, b) for a, b in zip(expand_aes_key(k), expand_aes128_key(k)))
    assert len(expand_aes_key(k)) == 11
    for n in (0, 15, 17, 20, 31, 33, 64):
        with pytest.raises(ValueError):
            expand_aes_key(np.zeros(n, np.uint8))
    with pytest.raises(ValueError):
        expand_aes_key(np.zeros((2, 16), np.uint8))


def test_block_functions_take_three_key_counts():
    from aes_keyschedule import expand_aes_key
    from ctr_mode import fips_block_fn, ref_block_fn
    from oracle import aes_plain as A
    rng = np.random.default_rng(0x256)
    pt = rng.integers(0, 256, 16).astype(np.uint8)
    rks = expand_aes_key(rng.integers(0, 256, 16).astype(np.uint8))
    # on 11 keys the two models are the oracle's two ciphers
    assert np.array_equal(ref_block_fn(rks)(pt), A.ref_encrypt(pt, rks))
    assert np.array_equal(fips_block_fn(rks)(pt), A.fips_encrypt(pt, rks))
    for n in (24, 32):
        rks = expand_aes_key(rng.integers(0, 256, n).astype(np.uint8))
        # the reference-order cipher from the oracle's own pieces, len(rks) - 1 rounds
        s = pt ^ rks[0]
        for r in range(1, len(rks) - 1):
            s = A.ref_mix_columns(A.shift_rows(A.SBOX[s])) ^ rks[r]
        assert np.array_equal(ref_block_fn(rks)(pt), A.shift_rows(A.SBOX[s]) ^ rks[-1]), n
        assert not np.array_equal(ref_block_fn(rks)(pt), fips_block_fn(rks)(pt))
    for fn in (fips_block_fn, ref_block_fn):
        for n in (10, 12, 14, 16):
            with pytest.raises(ValueError, match="11 round keys"):
                fn([np.zeros(16, np.uint8)] * n)


# ------------------------------------------------------------------ the 256-bit schedule's models
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("states,periodic", LAYOUTS)
def test_slot_plan_expands_256_bit_keys(states, periodic, order):
    """thirteen schedule_step_slots256 iterations from the two halves: all 15 round keys, a different key per state"""
    from aes_keyschedule import expand_aes_key
    from key_expansion import schedule_step_slots256
    enc = _encoder(states, periodic, order)
    keys = np.random.default_rng(0xA256 + states).integers(0, 256, (states, 32)).astype(np.uint8)
    keys[0] = np.arange(32, dtype=np.uint8)   # the C.3 key first
    half = lambda a: a[0] if states == 1 else a
    got = [enc.nibble_slots(half(keys[:, :16])), enc.nibble_slots(half(keys[:, 16:]))]
    for r in range(2, 15):
        got.append(schedule_step_slots256(got[-2], got[-1], r, enc.layout, enc.byte_order))
    assert len(got) == 15
    for b in range(states):
        want = expand_aes_key(keys[b])
        for r in range(15):
            dec = _bytes_of(enc, *got[r])
            assert np.array_equal(dec if states == 1 else dec[b], want[r]), (states, periodic, order, b, r)
    for r in (1, 15):
        with pytest.raises(ValueError):
            schedule_step_slots256(got[0], got[1], r, enc.layout, enc.byte_order)


@pytest.mark.parametrize("r", [2, 3])
def test_stage_byte_model_matches_the_slot_model_256(r):
    from aes_keyschedule import expand_aes_key
    from key_expansion import schedule_step_bytes256, schedule_step_slots256
    enc = _encoder(2, True, "transposed")
    keys = np.random.default_rng(30 + r).integers(0, 256, (2, 32)).astype(np.uint8)
    rks = [np.stack(k) for k in zip(*(expand_aes_key(k) for k in keys))]   # [r] -> (2, 16)
    stages = {}
    schedule_step_slots256(enc.nibble_slots(rks[r - 2]), enc.nibble_slots(rks[r - 1]), r, enc.layout, enc.byte_order, stages)
    want = schedule_step_bytes256(rks[r - 2], rks[r - 1], r)
    assert set(stages) == set(want) == {"prefix", "sub", "rot", "out"}
    for name in want:
        assert np.array_equal(_bytes_of(enc, *stages[name]), want[name]), name
    assert np.array_equal(want["out"], rks[r])
    one = schedule_step_bytes256(rks[r - 2][0], rks[r - 1][0], r)   # a (16,) key pair
    assert all(np.array_equal(one[name], want[name][0]) for name in want)
    with pytest.raises(ValueError):
        schedule_step_bytes256(rks[0], rks[1], 15)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("states,periodic", LAYOUTS + [(4, True)])
def test_wordcopy_sum(states, periodic, order):
    from key_expansion import SchedulePlan, word_pos
    from state_encoder import SlotLayout
    from utils import ZetaEncoder
    lay = SlotLayout(SLOTS, states, periodic)
    plan = SchedulePlan(lay, order)
    s = plan.wordcopy
    assert set(plan.sums256()) == {"shift1", "shift2", "broadcast", "wordcopy"} and plan.sums256()["wordcopy"] is s
    assert set(plan.sums()) == {"shift1", "shift2", "broadcast"}            # the 128-bit step's, unchanged
    used = plan.used() > 0.5
    cover = np.sum(s.masks, axis=0)
    fill = s.fill if s.fill is not None else np.zeros(SLOTS)
    for v in (*s.masks, fill):
        assert np.all((v == 0) | (v == 1))
    assert np.all(cover <= 1) and np.all(cover + fill == 1)                  # disjoint, and every slot accounted for
    assert np.all(cover[used] == 1) and not fill[used].any()                 # no fill on state slots
    assert np.all(fill[~used] == 1)
    assert 0 in s.steps and len(s.steps) == len(set(s.steps)) == 4           # the identity term: word 3 keeps itself
    assert all(st % lay.unit == 0 for st in s.steps)
    nib = np.random.default_rng(7).integers(0, 16, SLOTS).astype(np.uint8)
    got = s.apply_slots(nib)
    assert np.allclose(s.apply_values(ZetaEncoder.to_zeta(nib, 16)), ZetaEncoder.to_zeta(got, 16), atol=1e-12)
    # row rho of every word holds row rho of word 3, state by state (on the slot vector of real states)
    enc = _encoder(states, periodic, order)
    st = np.random.default_rng(8).integers(0, 256, (states, 16)).astype(np.uint8)
    _, lo = enc.nibble_slots(st[0] if states == 1 else st)
    before, after = enc._take(lo), enc._take(s.apply_slots(lo))   # (states, 16) by slot position
    for row in range(4):
        for word in range(4):
            assert np.array_equal(after[:, word_pos(row, word, order)], before[:, word_pos(row, 3, order)]), (row, word)
    if periodic:   # a periodic vector stays periodic: every tile holds the copy
        assert np.array_equal(s.apply_slots(lo)[:16 * lay.unit], s.apply_slots(lo)[-16 * lay.unit:])


def test_const_slots_and_rcon_slots():
    from aes_keyschedule import RCON
    from key_expansion import SchedulePlan
    from state_encoder import SlotLayout
    plan = SchedulePlan(SlotLayout(SLOTS, 1, True), "transposed")
    for r in range(1, 11):
        assert all(np.array_equal(a, b) for a, b in zip(plan.rcon_slots(r), plan.const_slots(r - 1)))
    hi, lo = plan.const_slots(6)   # the 256-bit schedule's last constant: r = 14 -> RCON[6]
    assert set(np.unique((hi << 4) | lo)) == {0, int(RCON[6])}
    for bad in (0, 11):
        with pytest.raises(ValueError):
            plan.rcon_slots(bad)
    for bad in (-1, 10):
        with pytest.raises(ValueError):
            plan.const_slots(bad)


# ------------------------------------------------------------------ containers and refusals
class _Ct:
    pass


@pytest.mark.parametrize("n", [13, 15])
def test_encrypted_round_keys_of_13_and_15(n):
    from key_expansion import EncryptedRoundKeys
    from state_encoder import SlotLayout
    lay = SlotLayout(SLOTS, 1, True)
    pairs = [(_Ct(), _Ct()) for _ in range(n)]
    erk = EncryptedRoundKeys.from_pairs(pairs, lay)
    assert len(erk) == n and erk[n - 1] == pairs[n - 1] and erk.packed == [None] * n and erk.key_basis == {}
    assert all(c.layout is lay for p in pairs for c in p)


def test_encrypted_round_keys_refuse_other_counts():
    from key_expansion import EncryptedRoundKeys
    from state_encoder import SlotLayout
    lay = SlotLayout(SLOTS, 1, True)
    for n in (10, 12, 14, 16):
        with pytest.raises(ValueError, match="11 round keys"):
            EncryptedRoundKeys.from_pairs([(_Ct(), _Ct()) for _ in range(n)], lay)


class _SeededEngine:
    """the import side of tests/test_seeded_ct.py's stand-in engine"""
    slot_count = 32

    def __init__(self):
        self.imports = []

    def import_half_many(self, rows, level, id0):
        rows = list(rows)
        self.imports.append((len(rows), level, id0))
        return [SimpleNamespace(level=level, b=r) for r in rows]


@pytest.mark.parametrize("n", [13, 15])
def test_load_seeded_of_26_and_30_records_is_one_import(n):
    from key_expansion import EncryptedRoundKeys
    from state_encoder import SlotLayout
    ctx = SimpleNamespace(engine=_SeededEngine())
    recs = [(np.full((3, 64), j, np.uint32), 5, None, (j << 16) | 0xBEEF) for j in range(2 * n)]
    erk = EncryptedRoundKeys.load_seeded(ctx, recs, SlotLayout(32, 1, False))
    assert ctx.engine.imports == [(2 * n, 5, 0xBEEF)]
    assert len(erk) == n and erk.packed == [None] * n
    assert [int(c.b[0, 0]) for pr in erk.pairs for c in pr] == list(range(2 * n))

    class _Exp:
        def export_half(self, ct):
            return ct.b, 0
    assert len(erk.dump_seeded(SimpleNamespace(engine=_Exp()))) == 2 * n


def test_load_seeded_refuses_other_counts():
    from key_expansion import EncryptedRoundKeys
    from state_encoder import SlotLayout
    ctx = SimpleNamespace(engine=_SeededEngine())
    b = np.zeros((3, 64), np.uint32)
    for n in (21, 24, 28, 32):
        with pytest.raises(ValueError, match="22 seeded records"):
            EncryptedRoundKeys.load_seeded(ctx, [(b, 5, None, 0)] * n, SlotLayout(32, 1, False))
    assert ctx.engine.imports == []


class _NoEngine:
    """a pipeline stand-in whose every attribute is a failure: the round-key count is checked before anything is used"""

    def __getattr__(self, name):
        raise AssertionError(f"the pipeline touched {name} before refusing the round keys")


@pytest.mark.parametrize("n", [10, 12, 14, 16])
def test_wrong_round_key_count_is_refused_before_any_engine_call(n):
    from pipeline import AESPipeline, round_count
    keys = [np.zeros(16, np.uint8)] * n
    nonce = bytes(12)
    calls = [
        lambda p: AESPipeline.encrypt(p, np.zeros(16, np.uint8), keys),
        lambda p: AESPipeline.decrypt(p, _Ct(), _Ct(), keys),
        lambda p: AESPipeline._prepare_round_keys(p, keys),
    ]
    for call in calls:
        with pytest.raises(ValueError, match="11 round keys"):
            call(_NoEngine())
    # the public-state entry points check pairs first (a plain attribute), then the count
    for name in ("encrypt_public", "ctr_keystream"):
        p = SimpleNamespace(pairs=1, _no_pairs=lambda what: None)
        with pytest.raises(ValueError, match="11 round keys"):
            getattr(AESPipeline, name)(p, *((np.zeros(16, np.uint8),) if name == "encrypt_public" else (nonce, 0)), keys)
    p = SimpleNamespace(pairs=1, _no_pairs=lambda what: None)
    with pytest.raises(ValueError, match="11 round keys"):
        AESPipeline.transcipher(p, np.zeros((1, 16), np.uint8), nonce, 0, keys)
    assert [round_count([0] * k) for k in (11, 13, 15)] == [10, 12, 14]


def test_encrypt_key_shapes_without_an_engine():
    """a 32-byte key is two 16-byte encodes (one batched call when seeded), a 24-byte key a ValueError naming AES-192"""
    from pipeline import AESPipeline
    seen = []

    class Enc:
        def encode(self, state, seeded=False):
            seen.append(("encode", np.array(state), seeded))
            return ("hi%d" % len(seen), "lo%d" % len(seen))

        def encode_many(self, states, seeded=False):
            seen.append(("encode_many", [np.array(s) for s in states], seeded))
            return [("hi0", "lo0"), ("hi1", "lo1")]

    key = np.arange(32, dtype=np.uint8)
    p = SimpleNamespace(pairs=1, states=1, encoder=Enc())
    assert AESPipeline.encrypt_key(p, key) == ("hi1", "lo1", "hi2", "lo2")
    assert [s[0] for s in seen] == ["encode", "encode"]
    assert np.array_equal(seen[0][1], key[:16]) and np.array_equal(seen[1][1], key[16:])
    seen.clear()
    assert AESPipeline.encrypt_key(p, key, seeded=True) == ("hi0", "lo0", "hi1", "lo1")
    assert len(seen) == 1 and seen[0][0] == "encode_many" and seen[0][2] is True
    assert np.array_equal(seen[0][1][0], key[:16]) and np.array_equal(seen[0][1][1], key[16:])
    # one key per state, and a shared key broadcast to every state
    seen.clear()
    p3 = SimpleNamespace(pairs=1, states=3, encoder=Enc())
    keys = np.random.default_rng(1).integers(0, 256, (3, 32)).astype(np.uint8)
    AESPipeline.encrypt_key(p3, keys)
    assert np.array_equal(seen[0][1], keys[:, :16]) and np.array_equal(seen[1][1], keys[:, 16:])
    seen.clear()
    AESPipeline.encrypt_key(p3, key)
    assert seen[1][1].shape == (3, 16) and np.array_equal(seen[1][1][2], key[16:])
    with pytest.raises(ValueError, match="AES-192"):
        AESPipeline.encrypt_key(p, np.zeros(24, np.uint8))
    with pytest.raises(ValueError, match="AES-192"):
        AESPipeline.encrypt_key(p3, np.zeros((3, 24), np.uint8))
    with pytest.raises(ValueError):
        AESPipeline.encrypt_key(p, np.zeros((2, 32), np.uint8))
