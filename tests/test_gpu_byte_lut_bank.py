"""A bank of byte tables with a table per slot (aesfhe_byte_lut_bank_public) against today's single-table
op, the CPU oracle and the float64 model gain * tables[select, m].

* the bank of one, and a bank of three under a constant selector, are aesfhe_byte_lut_public bit for bit;
* encode parity of all 16 x 9 rows under a selector drawn per slot, and all 16 outputs U_q bit-exact against the oracle MAC;
* the refusals, and an intact call after them;
* AESPipeline.to_lut_bank at log N 15 on 16 states covering all 256 byte values: T = 14 tables, K = 4 outputs, both layouts;
* AESPipeline.transcipher_lut_bank on the C2 set of tests/test_gpu_ctr.py (fips, 4 states across the 2^32 counter wrap) and
  on the 11 / 4 true-FHE set.

Error bound per slot, against the float64 model (never the code under test): test_gpu_byte_lut's
    B_f = (0.25 / 256) * S_f / S_id + 6e-4 * max|gain|
with f the SLOT'S OWN table and max|gain| the output's; slots without a state are asked the second term alone.  The
measured figures are in DESIGN.md §3.26.
"""
import numpy as np
import pytest

from test_byte_lut import TABLES, X
from test_gpu_byte_lut import FLOOR, _centred, _operands, _weights, pairs15, pipes15  # noqa: F401
from test_gpu_lut import rand_ct
from test_gpu_xor_value import NONCE, _block_fn, co, ctx9, rks, small  # noqa: F401

pytestmark = pytest.mark.gpu

I8 = X - 256 * (X >= 128)
ZPS = (-64, -7, 0, 5, 40, 100)


def relu_zp(zp):
    """relu(q - zp) of the byte read as int8, clipped to int8 and / 128"""
    return np.clip(I8 - zp, 0, 127) / 128.0


BITS = [((X >> k) & 1).astype(np.float64) for k in range(8)]
T14 = np.stack([relu_zp(zp) for zp in ZPS] + BITS)  # T = 14: six per-channel ReLUs, then the eight bit tables


def _Ks(tables):
    from coeffgen import byte_value_table
    return np.stack([byte_value_table(f)[0] for f in tables])


def _bank3():
    return _Ks([TABLES["random"], TABLES["mulaw"], TABLES["relu"]])


def _same(E, got, want):
    assert len(got) == len(want) == 16
    for g, (a, b) in enumerate(zip(got, want)):
        assert a.level == b.level, g
        assert np.array_equal(E.export(a), E.export(b)), g


def test_bank_of_one_is_todays_op(small):
    """log N 13: debug rows, scales and all 16 exports equal aesfhe_byte_lut_public's word for word -- for the bank of one
    with sel = 0, and for a bank of three under the constant selector t against the single table t"""
    E, O = small
    rng = np.random.default_rng(271)
    a_hi, l = _operands(E, O, rng, 6)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    w = _weights(E, rng)
    K3 = _bank3()
    zeros = np.zeros(E.slot_count, np.uint8)
    for bank, sel, single in [(K3[:1], zeros, K3[0])] + [(K3, np.full(E.slot_count, t, np.uint8), K3[t]) for t in range(3)]:
        ref = E.debug_byte_lut_pt(nib[0], nib[1], single, w, l)
        got = E.debug_byte_lut_bank_pt(nib[0], nib[1], bank, sel, w, l)
        assert np.array_equal(got[0], ref[0]) and got[1:] == ref[1:]
        _same(E, E.byte_lut_bank_public(a_hi, nib[0], nib[1], bank, sel, w), E.byte_lut_public(a_hi, nib[0], nib[1], single, w))


@pytest.fixture(scope="module")
def mixed(small):
    """(nibbles, selector drawn uniformly per slot, weights with zeros, the bank of three) at log N 13"""
    E, _ = small
    rng = np.random.default_rng(272)
    nib = [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(2)]
    sel = rng.integers(0, 3, E.slot_count).astype(np.uint8)
    assert set(np.unique(sel)) == {0, 1, 2}
    return nib, sel, _weights(E, rng), _bank3()


def test_bank_encode_parity(small, mixed):
    """test_byte_lut_encode_parity's check with T = 3 and a selector per slot: every device row at level 2 against
    OracleParams.encode(w * K[sel, p, g, b]) -- rows p = 1..8 at the plaintext scale, the fills at the product scale.  At
    most 1 per coefficient, the same integer on every limb"""
    E, O = small
    nib, sel, w, K = mixed
    level = 2
    nl = E.nl(level)
    rows, scale, fill_scale = E.debug_byte_lut_bank_pt(nib[0], nib[1], K, sel, w, level)
    assert rows.shape == (16, 9, nl, O.n)
    assert fill_scale > scale * 2.0 ** 28  # the product scale: ciphertext scale x plaintext scale
    b = 16 * nib[0].astype(np.int64) + nib[1]
    t = sel.astype(np.int64)
    q = O.limbs_mod(nl).astype(np.int64).reshape(-1, 1)
    worst = {0: 0, 1: 0}
    bad = []
    for g in range(16):
        for p in range(9):
            sc = fill_scale if p == 0 else scale
            dev = O.intt(rows[g, p], range(nl)).astype(np.int64)
            ref = O.intt(O.encode(w * K[t, p, g, b], sc, nl), range(nl)).astype(np.int64)  # encode returns NTT form
            d = _centred(dev - ref, q)
            assert bool(np.any(dev)) == bool(np.any(w * K[t, p, g, b]))  # a row of the support is not empty, the others are
            worst[p != 0] = max(worst[p != 0], int(np.abs(d).max()))
            if np.abs(d).max() > 1 or not np.all(d == d[0]):
                bad.append((g, p, int(np.abs(d).max()), bool(np.all(d == d[0]))))
    print(f"log N {O.log_n}, T = 3, mixed selector: max |device - oracle| coefficient = {worst[1]} at scale 2^{np.log2(scale):.2f} "
          f"(p = 1..8), {worst[0]} at the product scale 2^{np.log2(fill_scale):.2f} (the fills)")
    assert not bad, bad[:8]


def test_bank_mac_bitexact(small, mixed):
    """test_byte_lut_mac_bitexact's check through the bank op with the mixed selector: every U_q equals
    sum_p export(a_p) (.) P[q, p] + P[q, 0] on c0, mod q, put through the oracle's rescale, word for word: operands at
    level 6 and 5, one owing a rescale; weights with zeros"""
    E, O = small
    nib, sel, w, K = mixed
    assert (w == 0.0).any()
    a_hi, l = _operands(E, O, np.random.default_rng(273), 6)
    U = E.byte_lut_bank_public(a_hi, nib[0], nib[1], K, sel, w)
    assert len(U) == 16
    P = E.debug_byte_lut_bank_pt(nib[0], nib[1], K, sel, w, l)[0]
    nl = E.nl(l)
    q = O.limbs_mod(nl).astype(np.uint64).reshape(1, -1, 1)
    ops = [E.export(a if a.level == l else E.level_down(a, l)).astype(np.uint64) for _, a in sorted(a_hi.items())]
    for g, u in enumerate(U):
        assert u.level == l - 1
        acc = np.zeros((2, nl, O.n), np.uint64)
        for p, a in enumerate(ops, start=1):
            acc = (acc + a * P[g, p][None].astype(np.uint64) % q) % q
        acc[0] = (acc[0] + P[g, 0].astype(np.uint64)) % q[0]  # the fill joins c0
        assert np.array_equal(E.export(u), O.rescale(l, acc.astype(np.uint32))), g


def test_bank_errors(small):
    E, O = small
    rng = np.random.default_rng(274)
    sc = E.slot_count
    K = _bank3()
    T = len(K)
    nib = rng.integers(0, 16, sc).astype(np.uint8)
    sel = rng.integers(0, T, sc).astype(np.uint8)
    w = np.full(sc, 0.5)
    a_hi = {p: E.import_ct(rand_ct(O, 3, rng), 3) for p in range(1, 9)}
    bad = sel.copy()
    bad[sc // 2] = T
    with pytest.raises(RuntimeError, match="table index"):
        E.byte_lut_bank_public(a_hi, nib, nib, K, bad, w)
    with pytest.raises(RuntimeError, match="table index"):
        E.debug_byte_lut_bank_pt(nib, nib, K, bad, w, 2)
    with pytest.raises(RuntimeError, match="table index"):
        E.byte_lut_bank_public(a_hi, nib, nib, K[:1], np.full(sc, 1, np.uint8), w)  # the bank of one has table 0 alone
    with pytest.raises(RuntimeError, match="slot_count"):
        E.byte_lut_bank_public(a_hi, nib, nib, K, sel[:-1].copy(), w)
    with pytest.raises(RuntimeError, match="slot_count"):
        E.byte_lut_bank_public(a_hi, nib[:-1].copy(), nib[:-1].copy(), K, sel[:-1].copy(), w[:-1].copy())
    with pytest.raises(RuntimeError, match="table index"):
        E.byte_lut_bank_public(a_hi, nib, nib, K, None, w)  # a missing selector
    with pytest.raises(RuntimeError, match="table index"):
        E.debug_byte_lut_bank_pt(nib, nib, K, None, w, 2)
    with pytest.raises(RuntimeError, match="n_tables"):
        E.byte_lut_bank_public(a_hi, nib, nib, K[:0], sel, w)  # T = 0
    with pytest.raises(RuntimeError, match="n_tables"):
        E.byte_lut_bank_public(a_hi, nib, nib, np.tile(K[:1], (65, 1, 1, 1)), sel, w)  # T = 65
    Kbad = K.copy()
    Kbad[1, 4, 9, 77] = np.nan  # in the second table
    with pytest.raises(RuntimeError, match="not finite"):
        E.byte_lut_bank_public(a_hi, nib, nib, Kbad, sel, w)
    with pytest.raises(ValueError):
        E.byte_lut_bank_public(a_hi, nib, nib, K[0], sel, w)  # a single table is not a bank
    with pytest.raises(ValueError):
        E.byte_lut_bank_public(a_hi, nib, nib, K, sel.astype(np.int64), w)
    nb = nib.copy()
    nb[3] = 16
    with pytest.raises(RuntimeError, match="nibble"):
        E.byte_lut_bank_public(a_hi, nib, nb, K, sel, w)
    with pytest.raises(RuntimeError, match="missing weights"):
        E.byte_lut_bank_public(a_hi, nib, nib, K, sel, None)
    U = E.byte_lut_bank_public(a_hi, nib, nib, K, sel, w)  # the handles are intact after the refused calls
    assert [u.level for u in U] == [2] * 16


def _bounds(tables):
    """(S_f / S_id term of B_f per table, the smallest step between two distinct entries per table), on the CPU"""
    from coeffgen import byte_value_sensitivity
    s_id = byte_value_sensitivity(TABLES["identity"])
    first = np.array([(0.25 / 256.0) * byte_value_sensitivity(f) / s_id for f in tables])
    step = np.array([np.diff(np.unique(f)).min() for f in tables])
    return first, step


def _check(enc, ct, tables, select, m, gain, what):
    """per slot |decoded - gain tables[select, m]| <= B_f of the slot's own table on state slots, <= the floor term
    elsewhere; the largest errors are printed first.  Where a table's step exceeds 2 B_f / min|gain|, rounding
    decoded / gain to the nearest table entry must be exact too"""
    tables = np.asarray(tables)
    select = np.broadcast_to(select, m.shape)
    gain = np.broadcast_to(np.asarray(gain, np.float64), m.shape)
    top = float(np.abs(gain).max())
    first, step = _bounds(tables)
    bound = first[select] + FLOOR * top
    z = enc.ctx.decrypt(ct)
    got = enc.values_from_slots(z, "lut").reshape(m.shape)
    want = gain * tables[select, m]
    err = np.abs(got - want)
    rest = enc._float_slots(np.ones(m.shape)) == 0.0
    stray = float(np.abs(z[rest]).max()) if rest.any() else 0.0
    print(f"{what}: max error {err.max():.3g} slot units (bounds {bound.min():.3g}..{bound.max():.3g}, worst error / bound "
          f"{(err / bound).max():.3g}), slots without a state {stray:.3g} (bound {FLOOR * top:.3g}), max |imag| {np.abs(z.imag).max():.3g}")
    assert enc.decode_values(ct).shape == ((16,) if enc.states == 1 else m.shape)
    assert ct.value_dtype == "lut"
    assert np.all(err <= bound)
    assert stray <= FLOOR * top
    exact = step[select] > 2.0 * bound / np.abs(gain).min()  # the slot's own table: rounding cannot miss
    snapped = np.rint(got / gain / step[select]) * step[select]
    assert np.array_equal(snapped[exact], (np.rint(tables[select, m] / step[select]) * step[select])[exact])
    return float(err.max()), bool(exact.all())


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "reference"])
def test_to_lut_bank_logn15(pipes15, pairs15, periodic):
    """T = 14, K = 4: output 0 takes relu_zp[i % 6] at byte position i under a random gain in +-[0.5, 1]; outputs 1..3 are
    bits 0, 3 and 7 of every byte at gain 1.  All fourteen tables' steps (1 / 128 and 1) exceed 2 B_f / min|gain|: every
    slot must round to its table entry exactly"""
    import mi355x_ckks
    from utils import BYTE_LUT_DEPTH
    pipe = pipes15[periodic]
    m, pairs = pairs15
    hi, lo = pairs[periodic]
    first, _ = _bounds(T14)
    assert np.all((first + FLOOR > 0.0009) & (first + FLOOR < 0.0018))
    rng = np.random.default_rng(275)
    gains = [rng.uniform(0.5, 1.0, (16, 16)) * rng.choice([-1.0, 1.0], (16, 16)), 1.0, 1.0, 1.0]
    selects = [np.arange(16) % 6, 6 + 0, 6 + 3, 6 + 7]
    n0 = mi355x_ckks.launch_count()
    outs = pipe.to_lut_bank(hi, lo, T14, selects, gains)
    pipe.ctx.engine.settle(*outs)
    launches = mi355x_ckks.launch_count() - n0
    assert len(outs) == 4
    layout = "periodic" if periodic else "reference"
    for k, out in enumerate(outs):
        assert out.level == hi.level - BYTE_LUT_DEPTH
        _, exact = _check(pipe.encoder, out, T14, selects[k], m, gains[k], f"to_lut_bank log N 15, 16 states, {layout} layout, output {k}")
        assert exact  # the rounding check covered every slot
    print(f"launch census, to_lut_bank at log N 15, K = 4 outputs: {launches} launches")


def test_transcipher_lut_bank_fips_wrap(ctx9, co, rks):
    """C2 set, fips=True (transposed bytes), 4 states across the 2^32 counter wrap, tables [relu_zp(0), relu_zp(40),
    mulaw]: output 0 selects by byte position i % 2, output 1 is mu-law everywhere; both at keystream level - 5 == 2.

    Output 1 against transcipher_lut(..., mulaw): the two calls evaluate the keystream separately, and every secret-key
    renorm inside it re-encrypts with randomness drawn from the engine's advancing encryption counter (pool emptied or
    not), so the two keystreams are different ciphertexts of the same bytes and their exports differ.  What holds, and is
    asserted, is (a) the decoded slots of the two calls within 2 B_f, and (b) on ONE shared keystream the bank's output
    and ByteValueLUT's are the same ciphertext word for word (np.array_equal of the exports)."""
    import mi355x_ckks
    from ctr_mode import ctr_xor, fips_block_fn
    from pipeline import AESPipeline
    from utils import BYTE_LUT_DEPTH
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True, states=4)
    eng = ctx9.engine
    rng = np.random.default_rng(276)
    m = rng.integers(0, 256, (4, 16)).astype(np.uint8)
    m[0, :8] = [0x00, 0x80, 0xFF, 0x7F, 0x01, 0x81, 0xFE, 0x7E]
    c0 = 2 ** 32 - 2
    c = ctr_xor(fips_block_fn(rks), m, NONCE, c0)
    tables = np.stack([relu_zp(0), relu_zp(40), TABLES["mulaw"]])
    selects = [np.arange(16) % 2, 2]
    gains = [rng.uniform(0.5, 1.0, 16), 1.0]
    ks_level = pipe.ctr_keystream(NONCE, c0, rks)[0].level
    eng.renorm_pool(-1)  # every pool emptied, the size kept
    outs = pipe.transcipher_lut_bank(c, NONCE, c0, rks, tables, selects, gains)
    assert len(outs) == 2
    for k, out in enumerate(outs):
        assert out.level == ks_level - BYTE_LUT_DEPTH == 2
        _check(pipe.encoder, out, tables, selects[k], m, gains[k], f"transcipher_lut_bank, C2 set, fips, 4 states across the wrap, output {k}")
    eng.renorm_pool(-1)
    single = pipe.transcipher_lut(c, NONCE, c0, rks, TABLES["mulaw"])
    first, _ = _bounds(tables)
    same = np.array_equal(eng.export(outs[1]), eng.export(single))
    diff = float(np.abs(pipe.encoder.decode_values(outs[1]) - pipe.encoder.decode_values(single)).max())
    print(f"output 1 vs transcipher_lut(mulaw): exports equal {same}, decoded slots differ by {diff:.3g} (bound 2 B_f = {2 * (first[2] + FLOOR):.3g})")
    assert diff <= 2.0 * (first[2] + FLOOR)
    ks = pipe.ctr_keystream(NONCE, c0, rks)
    nib = pipe.encoder.nibble_slots(c)
    eng.settle(*ks)
    one = pipe._byte_lut(TABLES["mulaw"], 1.0).apply_public(*ks, *nib)
    got = pipe._byte_bank(tables, selects[1:], 1.0).apply_public(*ks, *nib)
    assert len(got) == 1 and np.array_equal(eng.export(got[0]), eng.export(one))
    # launch census of the last step alone (printed, not asserted)
    census = []
    for K in (1, 2):
        bank = pipe._byte_bank(tables, selects[:K], gains[:K])
        n0 = mi355x_ckks.launch_count()
        eng.settle(*bank.apply_public(*ks, *nib))
        census.append(mi355x_ckks.launch_count() - n0)
    n0 = mi355x_ckks.launch_count()
    eng.settle(pipe._byte_lut(TABLES["mulaw"], 1.0).apply_public(*ks, *nib))
    print(f"launch census, last step on the C2 set: transcipher_lut_bank K = 1 {census[0]} launches, K = 2 {census[1]} launches, "
          f"transcipher_lut {mi355x_ckks.launch_count() - n0} launches")


def test_transcipher_lut_bank_true_fhe(co, rks, monkeypatch):
    """the 11 / 4 true-FHE set: one block, K = 2 (mu-law and bit 7), the keystream's own bootstrap + snap the last renorm
    and no secret-key call between the key's encryption and the outputs"""
    from ctr_mode import ctr_xor
    from engine_context import EngineContext
    from pipeline import AESPipeline
    from test_gpu_true_fhe import _no_secret_renorm
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    pipe = AESPipeline(c12, co, use_hard_renorm_between_steps=False, true_fhe=True)
    assert pipe.encoder.renorm_hook is not None
    m = np.random.default_rng(279).integers(0, 256, (1, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 7)
    tables = np.stack([TABLES["mulaw"], BITS[7]])
    pipe._prepare_round_keys(rks)  # the key's encryption is the client's part
    _no_secret_renorm(c12, monkeypatch)
    outs = pipe.transcipher_lut_bank(c[0], NONCE, 7, rks, tables, [0, 1])
    monkeypatch.undo()
    assert len(outs) == 2
    for k, out in enumerate(outs):
        _check(pipe.encoder, out, tables, k, m, 1.0, f"transcipher_lut_bank, true-FHE 11 / 4 set, output {k}")
