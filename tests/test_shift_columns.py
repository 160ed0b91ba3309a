"""ShiftColumns (shift_columns.py): the byte model, the transposed-state identity behind AESPipeline(fips=True),
the cell masks, and the masked-rotation forms on plain numpy slot vectors (np.roll = the engine's rotate)."""
import numpy as np
import pytest

SC = [0, 1, 2, 3, 5, 6, 7, 4, 10, 11, 8, 9, 15, 12, 13, 14]
INV_SC = [0, 1, 2, 3, 7, 4, 5, 6, 10, 11, 8, 9, 13, 14, 15, 12]
SLOTS = 4096


def test_tables_and_byte_model():
    from shift_columns import INV_SC_PERM, SC_PERM, shift_columns_bytes, transpose_bytes
    from oracle import aes_plain
    assert SC_PERM == SC and INV_SC_PERM == INV_SC
    ident = np.arange(16, dtype=np.uint8)
    assert shift_columns_bytes(ident, -1).tolist() == SC
    assert shift_columns_bytes(ident, +1).tolist() == INV_SC
    assert [SC[INV_SC[i]] for i in range(16)] == list(range(16)) == [INV_SC[SC[i]] for i in range(16)]
    rng = np.random.default_rng(0)
    s = rng.integers(0, 256, (5, 16)).astype(np.uint8)
    assert np.array_equal(shift_columns_bytes(shift_columns_bytes(s, -1), +1), s)
    assert np.array_equal(shift_columns_bytes(s, -1)[3], shift_columns_bytes(s[3], -1))
    # SC = T . ShiftRows . T, and its inverse likewise
    for x in s:
        assert np.array_equal(shift_columns_bytes(x, -1), transpose_bytes(aes_plain.shift_rows(transpose_bytes(x))))
        assert np.array_equal(shift_columns_bytes(x, +1), transpose_bytes(aes_plain.inv_shift_rows(transpose_bytes(x))))
    assert np.array_equal(transpose_bytes(transpose_bytes(s)), s)
    assert transpose_bytes(ident).tolist() == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]


def test_slot_perm_tables():
    from shift_columns import InvShiftColumns, ShiftColumns
    from state_encoder import SlotLayout
    ctx = _NumpyCtx(SLOTS)
    one = SlotLayout(SLOTS, 1, periodic=True)
    assert ShiftColumns(ctx, layout=one).slot_perm() == SC
    assert InvShiftColumns(ctx, layout=one).slot_perm() == INV_SC
    assert ShiftColumns(ctx, layout=one).direction == -1 and InvShiftColumns(ctx, layout=one).direction == +1
    assert ShiftColumns(ctx, layout=one).layout is one
    assert ShiftColumns(ctx, states=4, layout=SlotLayout(SLOTS, 4, periodic=True)).slot_perm() is None
    assert ShiftColumns(ctx, layout=SlotLayout(SLOTS, 1)).slot_perm() is None


def _e_prime(s, rks, direction=-1):
    """the pipeline's round sequence on bytes with ShiftColumns in place of ShiftRows (row-mixing MixColumns)"""
    from shift_columns import shift_columns_bytes
    from oracle import aes_plain as ap
    s = np.asarray(s, np.uint8) ^ rks[0]
    for r in range(1, 10):
        s = ap.ref_mix_columns(shift_columns_bytes(ap.SBOX[s], -1)) ^ rks[r]
    return shift_columns_bytes(ap.SBOX[s], -1) ^ rks[10]


def _d_prime(c, rks):
    """its inverse: InvShiftColumns, InvSubBytes, AddRoundKey, the row-mixing InvMixColumns"""
    from shift_columns import shift_columns_bytes
    from oracle import aes_plain as ap
    s = np.asarray(c, np.uint8) ^ rks[10]
    for r in range(9, 0, -1):
        s = ap.ref_inv_mix_columns(ap.INV_SBOX[shift_columns_bytes(s, +1)] ^ rks[r])
    return ap.INV_SBOX[shift_columns_bytes(s, +1)] ^ rks[0]


def _fips_via_transpose(p, rks):
    from shift_columns import transpose_bytes as T
    return T(_e_prime(T(p), [T(k) for k in rks]))


def _fips_decrypt_via_transpose(c, rks):
    from shift_columns import transpose_bytes as T
    return T(_d_prime(T(c), [T(k) for k in rks]))


def test_transposed_state_identity():
    from ctr_mode import fips_block_fn
    from oracle import aes_plain as ap
    rng = np.random.default_rng(0xF1)
    for _ in range(20):
        rks = ap.expand_key(rng.integers(0, 256, 16).astype(np.uint8))
        p = rng.integers(0, 256, 16).astype(np.uint8)
        c = ap.fips_encrypt(p, rks)
        assert np.array_equal(_fips_via_transpose(p, rks), c)
        assert np.array_equal(_fips_decrypt_via_transpose(c, rks), p)
        assert np.array_equal(fips_block_fn(rks)(p), c)
    # FIPS-197 Appendix B and Appendix C.1
    for key, pt, ct in (("2b7e151628aed2a6abf7158809cf4f3c", "3243f6a8885a308d313198a2e0370734", "3925841d02dc09fbdc118597196a0b32"),
                        ("000102030405060708090a0b0c0d0e0f", "00112233445566778899aabbccddeeff", "69c4e0d86a7b0430d8cdb78070b4c55a")):
        rks = ap.expand_key(np.frombuffer(bytes.fromhex(key), np.uint8))
        p, c = np.frombuffer(bytes.fromhex(pt), np.uint8), np.frombuffer(bytes.fromhex(ct), np.uint8)
        assert bytes(_fips_via_transpose(p, rks)).hex() == ct
        assert bytes(_fips_decrypt_via_transpose(c, rks)).hex() == pt
        assert bytes(fips_block_fn(rks)(p)).hex() == ct


def test_ctr_xor_over_fips_block_fn_is_sp800_38a():
    """SP 800-38A F.5.1 (CTR-AES128.Encrypt), blocks 1 and 2: the 16-byte initial counter block as nonce12 + counter"""
    from ctr_mode import ctr_xor, fips_block_fn
    from oracle import aes_plain as ap
    rks = ap.expand_key(np.frombuffer(bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"), np.uint8))
    icb = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
    pt = np.frombuffer(bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"), np.uint8).reshape(2, 16)
    out = ctr_xor(fips_block_fn(rks), pt, icb[:12], int.from_bytes(icb[12:], "big"))
    assert bytes(out[0]).hex() == "874d6191b620e3261bef6864990db6ce"
    assert bytes(out[1]).hex() == "9806f66b7970fdff8617187bb9fffdff"


@pytest.mark.parametrize("periodic", [False, True], ids=["reference", "periodic"])
@pytest.mark.parametrize("states", [1, 4])
def test_cell_masks_partition_the_state_slots(states, periodic):
    from state_encoder import SlotLayout
    lay = SlotLayout(SLOTS, states, periodic)
    cells = [lay.cell_mask(r, c) for c in range(4) for r in range(4)]
    total = np.sum(cells, axis=0)
    assert set(np.unique(total.real)) <= {0.0, 1.0} and not total.imag.any()
    assert np.array_equal(total, np.sum([lay.row_mask(r) for r in range(4)], axis=0))
    for r in range(4):  # each row mask is its four cells; existing masks are what they were
        assert np.array_equal(lay.row_mask(r), np.sum([lay.cell_mask(r, c) for c in range(4)], axis=0))
    assert int(total.real.sum()) == 16 * states * (SLOTS // lay.period)
    # cell (r, c) is byte r + 4c of every state
    j = np.flatnonzero(cells[6].real)
    assert np.array_equal((j % lay.period) // lay.unit, np.full(j.size, 6)) and ((j % lay.unit) < states).all()


def _slot_perm(lay, x, perm):
    """the byte permutation on a slot vector: byte i's slots take byte perm[i]'s"""
    j = np.arange(lay.sc)
    cell = (j % lay.period) // lay.unit
    return x[(j + (np.asarray(perm)[cell] - cell) * lay.unit) % lay.sc]


def _periodic_vec(lay, rng):
    return lay.tile(rng.random(lay.period) + 1j * rng.random(lay.period))


@pytest.mark.parametrize("direction", [-1, +1])
@pytest.mark.parametrize("states,periodic", [(1, False), (4, False), (1, True), (4, True)])
def test_apply_terms_reproduce_the_permutation(states, periodic, direction):
    from shift_columns import apply_terms
    from state_encoder import SlotLayout
    lay = SlotLayout(SLOTS, states, periodic)
    steps, masks = apply_terms(lay, direction)
    assert len(steps) == 7 and sum(1 for s in steps if s) == 6
    rng = np.random.default_rng(3)
    x = rng.random(SLOTS) + 1j * rng.random(SLOTS)
    if periodic:
        x = _periodic_vec(lay, rng)
    got = sum(m * np.roll(x, s) for m, s in zip(masks, steps))
    state = np.sum([lay.row_mask(r) for r in range(4)], axis=0).real
    want = _slot_perm(lay, x, SC if direction == -1 else INV_SC) * state
    assert np.allclose(got, want, atol=0, rtol=0)


@pytest.mark.parametrize("states", [1, 4])
def test_entry_terms_reproduce_both_packs(states):
    """the 11 steps and their masks give pack(SC(x)) and pack(rot(SC(x), s1)) for a periodic pair"""
    from shift_columns import entry_terms
    from state_encoder import SlotLayout
    lay = SlotLayout(SLOTS, states, periodic=True)
    steps, masks = entry_terms(lay, -1)
    assert len(steps) == 11 and sum(1 for s in steps if s) == 10
    for h in (0, 1):
        for o in (0, 1):
            assert sum(m is not None for m in masks[h][o]) == 7  # 14 masked terms per output over both halves
    rng = np.random.default_rng(4)
    x = [_periodic_vec(lay, rng), _periodic_vec(lay, rng)]
    s1 = -4 * lay.unit
    pack = lambda a, b: a * lay.half_mask(0) + b * lay.half_mask(1)  # noqa: E731
    sc = [_slot_perm(lay, v, SC) for v in x]
    want = [pack(*sc), pack(*[np.roll(v, s1) for v in sc])]
    for o in (0, 1):
        got = sum(m * np.roll(x[h], s) for h in (0, 1) for m, s in zip(masks[h][o], steps) if m is not None)
        assert np.allclose(got, want[o], atol=0, rtol=0)
    with pytest.raises(ValueError):
        entry_terms(SlotLayout(SLOTS, 1), -1)


class _NumpyCtx:
    """slot vectors as ciphertexts: encode / rot_pt_sum with np.roll, as the engine defines them"""

    class _Eng:
        def __init__(self, sc):
            self.slot_count = sc

    def __init__(self, sc):
        self.engine = self._Eng(sc)
        self.calls = []

    def encode(self, v):
        return np.asarray(v, np.complex128)

    def rot_pt_sum(self, ct, steps, pts_per_output):
        self.calls.append((len(steps), len(pts_per_output)))
        return [sum(p * np.roll(ct, s) for p, s in zip(pts, steps) if p is not None) for pts in pts_per_output]


@pytest.mark.parametrize("cls,perm", [("ShiftColumns", SC), ("InvShiftColumns", INV_SC)])
def test_module_apply_on_numpy_context(cls, perm):
    import shift_columns
    from state_encoder import SlotLayout
    ctx = _NumpyCtx(SLOTS)
    lay = SlotLayout(SLOTS, 2, periodic=True)
    mod = getattr(shift_columns, cls)(ctx, states=2, layout=lay)
    rng = np.random.default_rng(5)
    hi, lo = _periodic_vec(lay, rng), _periodic_vec(lay, rng)
    out = mod.apply(hi, lo)
    assert ctx.calls == [(7, 1), (7, 1)]
    assert np.allclose(out[0], _slot_perm(lay, hi, perm)) and np.allclose(out[1], _slot_perm(lay, lo, perm))


def test_layout_tag_keeps_transposed_pairs_apart():
    from state_encoder import SlotLayout, check_layout, tag_layout

    class Ct:
        pass

    plain, tr = SlotLayout(SLOTS, 1, True), SlotLayout(SLOTS, 1, True)
    tr.byte_order = "transposed"
    assert plain.same(SlotLayout(SLOTS, 1, True)) and not plain.same(tr) and not tr.same(plain) and tr.same(tr)
    c = Ct()
    tag_layout(tr, c)
    check_layout(tr, c)
    with pytest.raises(ValueError, match="transposed"):
        check_layout(plain, c)


def test_context_fallback_without_the_engine_entry_point():
    """EngineContext.rot_pt_sum on an engine that lacks rot_pt_sum: hoisted rotations, products and additions"""
    from engine_context import EngineContext

    class Eng:
        slot_count = 64

        def multiply(self, a, b):
            return a * b

        def add(self, a, b):
            return a + b

    class Stub:
        engine = Eng()
        calls = []

        def rotate_many(self, ct, steps):
            self.calls.append(list(steps))
            return [np.roll(ct, s) for s in steps]

    rng = np.random.default_rng(8)
    x = rng.random(64) + 1j * rng.random(64)
    steps = [0, 3, -2]
    pts = [[rng.random(64), None, rng.random(64)], [None, rng.random(64), None]]
    stub = Stub()
    out = EngineContext.rot_pt_sum(stub, x, steps, pts)
    assert stub.calls == [steps]  # one hoisted call for every output
    for o, row in zip(out, pts):
        assert np.allclose(o, sum(p * np.roll(x, s) for p, s in zip(row, steps) if p is not None))
