"""The pure-Python side of seeded symmetric encryption: the wire records of dump_ct_seeded /
load_ct_seeded, how consecutive ids are batched into one import, and the ValueErrors.  The engine is a stand-in that
records its calls; the device path is tests/test_gpu_seeded_ct.py's."""
from types import SimpleNamespace

import numpy as np
import pytest

SC, N, NL = 32, 64, 3


class _Ct:
    def __init__(self, level, seed_id=None, b=None):
        self.level, self.seed_id, self.b = level, seed_id, b


class _Engine:
    slot_count = SC

    def __init__(self):
        self.imports = []   # (batch, level, first id) of every import_half_many call
        self.ctr = 0

    def export_half(self, ct):
        if ct.seed_id is None:
            raise RuntimeError("export_half: not a seeded ciphertext")
        return ct.b, ct.seed_id

    def import_half_many(self, rows, level, id0):
        rows = list(rows)
        assert all(r.dtype == np.uint32 and r.ndim == 2 for r in rows)
        self.imports.append((len(rows), level, id0))
        return [_Ct(level, None, r) for r in rows]

    def encrypt_seeded_many(self, vecs, level=None):
        out = [_Ct(5 if level is None else level, ((self.ctr + j) << 16) | 0xBEEF, np.full((NL, N), self.ctr + j, np.uint32))
               for j in range(len(vecs))]
        self.ctr += len(vecs)
        return out


def _ctx():
    e = _Engine()
    return SimpleNamespace(engine=e, encrypt_seeded_many=e.encrypt_seeded_many, stack=lambda cts: cts)


def test_record_shape_and_round_trip():
    from state_encoder import SlotLayout, dump_ct_seeded, load_ct_seeded, tag_layout
    ctx = _ctx()
    ct = ctx.encrypt_seeded_many([None])[0]
    rec = dump_ct_seeded(ctx, ct)
    assert len(rec) == 4 and rec[0] is ct.b and rec[1:] == (5, None, 0xBEEF)
    lay = SlotLayout(SC, 1, True)
    lay.byte_order = "transposed"
    tag_layout(lay, ct)
    b, level, tag, sid = dump_ct_seeded(ctx, ct)
    assert tag == dict(sc=SC, states=1, periodic=True, byte_order="transposed")
    back = load_ct_seeded(ctx, b, level, sid, tag)
    assert ctx.engine.imports == [(1, 5, 0xBEEF)] and np.array_equal(back.b, b)
    assert back.layout.same(lay) and back.layout.byte_order == "transposed"
    assert not hasattr(load_ct_seeded(ctx, b, level, sid), "layout")
    with pytest.raises(RuntimeError, match="not a seeded ciphertext"):
        dump_ct_seeded(ctx, back)


def test_consecutive_ids_share_an_import():
    from state_encoder import dump_ct_seeded, load_cts_seeded
    ctx = _ctx()
    recs = [dump_ct_seeded(ctx, c) for c in ctx.encrypt_seeded_many([None] * 3)]
    recs += [dump_ct_seeded(ctx, c) for c in ctx.encrypt_seeded_many([None] * 2, level=1)]   # ids go on, the level does not
    skip = ctx.encrypt_seeded_many([None] * 2)[1]                                            # a gap of one id
    recs.append(dump_ct_seeded(ctx, skip))
    out = load_cts_seeded(ctx, recs)
    assert ctx.engine.imports == [(3, 5, 0xBEEF), (2, 1, (3 << 16) | 0xBEEF), (1, 5, (6 << 16) | 0xBEEF)]
    assert [int(c.b[0, 0]) for c in out] == [0, 1, 2, 3, 4, 6]


def test_value_errors():
    from key_expansion import EncryptedRoundKeys
    from pipeline import AESPipeline
    from state_encoder import SlotLayout, StateEncoder, load_ct_seeded
    ctx = _ctx()
    b = np.zeros((NL, N), np.uint32)
    with pytest.raises(ValueError, match="slots into a context"):
        load_ct_seeded(ctx, b, 5, 0, dict(sc=2 * SC, states=1, periodic=False))
    with pytest.raises(ValueError, match=r"\[limbs\]\[N\]"):
        load_ct_seeded(ctx, np.zeros((2, NL, N), np.uint32), 5, 0)
    assert ctx.engine.imports == []
    with pytest.raises(ValueError, match="22 seeded records"):
        EncryptedRoundKeys.load_seeded(ctx, [(b, 5, None, 0)] * 21, SlotLayout(SC, 1, False))
    enc = StateEncoder(SimpleNamespace(engine=SimpleNamespace(slot_count=64), stack=lambda c: c), pairs=2)
    with pytest.raises(ValueError, match="pairs > 1"):
        enc.encode(np.zeros((2, 16), np.uint8), seeded=True)
    with pytest.raises(ValueError, match="pairs > 1"):
        enc.encode_many([np.zeros((2, 16), np.uint8)], seeded=True)
    one = StateEncoder(SimpleNamespace(engine=SimpleNamespace(slot_count=64)))
    with pytest.raises(ValueError, match="encrypt_seeded_many"):
        one.encode(np.zeros(16, np.uint8), seeded=True)        # a context with no seeded encryption
    with pytest.raises(ValueError, match="pairs > 1"):
        AESPipeline.encrypt_key(SimpleNamespace(pairs=2), np.zeros(16, np.uint8), seeded=True)


def test_seeded_encode_is_one_batched_call():
    from state_encoder import StateEncoder
    e = _Engine()
    calls = []

    def many(vecs, level=None):
        calls.append(len(vecs))
        return e.encrypt_seeded_many(vecs, level)

    enc = StateEncoder(SimpleNamespace(engine=SimpleNamespace(slot_count=64), encrypt_seeded_many=many), periodic=True)
    hi, lo = enc.encode(np.arange(16, dtype=np.uint8), seeded=True)
    assert calls == [2] and lo.seed_id == hi.seed_id + (1 << 16) and enc.layout.same(hi.layout)
    pairs = enc.encode_many([np.arange(16, dtype=np.uint8)] * 11, seeded=True)
    assert calls == [2, 22] and len(pairs) == 11
    assert [c.seed_id >> 16 for pr in pairs for c in pr] == list(range(2, 24))


def test_a_plain_ciphertext_has_no_seed_id():
    from mi355x_ckks import Ciphertext
    c = Ciphertext(None, 0)
    assert c.seed_id is None
    c._seed_id = 7 << 16
    assert c.seed_id == 7 << 16
