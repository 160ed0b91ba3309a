"""AES-192 / AES-256 in AESPipeline and the homomorphic AES-256 key schedule on the C2 set of
tests/test_gpu_key_expansion.py (boot_fresh_level=7, dnum=4): the round count follows the round keys (11 / 13 / 15 keys
run 10 / 12 / 14 rounds), expand_key(*encrypt_key(key32)) derives the 15 AES-256 round keys from an encrypted 32-byte key.

References: aes_keyschedule.expand_aes_key, key_expansion.schedule_step_bytes256 for the debug stages, FIPS-197
Appendix C.1 - C.3, ctr_mode.ctr_xor over fips_block_fn / ref_block_fn.  Precision: the largest slot error of any
expanded key must sit at least 100x inside the decode margin pi / 16, the margin tests/test_gpu_key_expansion.py asks of
the AES-128 expansion.  Every test prints what it measures (time, launches, renorms, margin); DESIGN.md §3.30 records
them.  Measured on an MI355X: largest slot error of any of the 15 expanded keys 3.4e-5 rad with fips=True (5771x inside
pi / 16); transcipher_values under expanded AES-256 keys, two states: 0.011 byte units (rounding margin 0.5)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PT = bytes.fromhex("00112233445566778899aabbccddeeff")
C1_CT = "69c4e0d86a7b0430d8cdb78070b4c55a"   # FIPS-197 C.1, key 00..0f
C2_CT = "dda97ca4864cdfe06eaf70a0ec0d7191"   # FIPS-197 C.2, key 00..17
C3_CT = "8ea2b7ca516745bfeafc49904b496089"   # FIPS-197 C.3, key 00..1f
MASK = bytes(range(0xA0, 0xC0))              # the public mask key of tests/test_gpu_seeded_ct.py: seeded encryption needs one


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


KEY16, KEY24, KEY32 = (_u8(range(n)) for n in (16, 24, 32))


@pytest.fixture(scope="module")
def ctx9():
    from engine_context import EngineContext
    return EngineContext(signature=1, boot_fresh_level=7, dnum=4, thread_count=4, seed=0xC2C2, enc_nonce=0xC2C2, mask_key=MASK)


@pytest.fixture(scope="module")
def co(coeff_dir):
    from aes_keyschedule import load_all_coeffs
    return load_all_coeffs(coeff_dir)


@pytest.fixture(scope="module")
def rks():
    """{key bytes: clear round keys} of the three Appendix C keys, computed once"""
    from aes_keyschedule import expand_aes_key
    return {n: expand_aes_key(k) for n, k in ((16, KEY16), (24, KEY24), (32, KEY32))}


@pytest.fixture(scope="module")
def pipe(ctx9, co):
    from pipeline import AESPipeline
    return AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True)


def _expand(p, key):
    """(EncryptedRoundKeys, debug stages) with the expansion's time, launches and renorms printed"""
    import mi355x_ckks
    from utils import RENORM_TALLY
    ck = p.encrypt_key(key)
    assert len(ck) == 4
    p.ctx.engine.sync()
    dbg = {}
    n0, r0, t0 = mi355x_ckks.launch_count(), RENORM_TALLY["calls"], time.perf_counter()
    erk = p.expand_key(*ck, debug=dbg)
    p.ctx.engine.sync()
    dt = time.perf_counter() - t0
    print(f"AES-256 expand_key fips {int(p.fips)} states {p.states} (with debug decodes): {dt:.3f} s, "
          f"{mi355x_ckks.launch_count() - n0} launches, {RENORM_TALLY['calls'] - r0} secret-key renorm calls")
    return erk, dbg


@pytest.fixture(scope="module")
def expanded(pipe):
    return _expand(pipe, KEY32)


def test_expansion_fips(pipe, expanded, rks):
    from key_expansion import EncryptedRoundKeys, schedule_step_bytes256
    from utils import ZetaEncoder
    erk, dbg = expanded
    want = rks[32]
    assert isinstance(erk, EncryptedRoundKeys) and len(erk) == 15
    enc = pipe.encoder
    err, fresh = 0.0, enc.encode(want[0])[0].level
    for r in range(15):
        got = enc.decode(*erk[r])
        assert np.array_equal(got, want[r]), (r, bytes(got).hex(), bytes(want[r]).hex())
        assert erk[r][0].level == erk[r][1].level == fresh  # the level _encode_key hands out
        held = enc._order(got[None, :])
        for c, nib in zip(erk[r], (held >> 4, held & 15)):
            z = enc._take(pipe.ctx.decrypt(c))
            err = max(err, float(np.abs(np.angle(z / ZetaEncoder.to_zeta(nib, 16))).max()))
    for r in (2, 3):  # one even step (constant, broadcast) and one odd step (no constant, word copy)
        stages = schedule_step_bytes256(want[r - 2], want[r - 1], r)
        for name in ("prefix", "sub", "rot", "out"):
            assert np.array_equal(dbg[f"ks.r{r}.{name}"]["plain"], stages[name]), (r, name)
    assert set(dbg) == {f"ks.r{r}.{s}" for r in range(2, 15) for s in ("prefix", "sub", "rot", "out")}
    margin = (np.pi / 16) / err
    print(f"AES-256 expanded keys fips 1: max slot error {err:.3g} rad, margin {margin:.0f}x inside pi/16")
    assert margin >= 100.0


def test_fips_encrypt_decrypt_with_expanded_keys(pipe, expanded):
    import mi355x_ckks
    erk, _ = expanded
    pipe.ctx.engine.sync()
    n0, t0 = mi355x_ckks.launch_count(), time.perf_counter()
    ct = pipe.encrypt(_u8(PT), erk)
    pipe.ctx.engine.sync()
    print(f"AES-256 encrypt under expanded keys (first call: packs the keys): {time.perf_counter() - t0:.3f} s, "
          f"{mi355x_ckks.launch_count() - n0} launches")
    assert bytes(pipe.encoder.decode(*ct)).hex() == C3_CT
    assert len(erk.packed) == 15 and all(k is not None for k in erk.packed[1:14]) and erk.packed[0] is None
    assert np.array_equal(pipe.encoder.decode(*pipe.decrypt(*ct, erk)), _u8(PT))


def test_default_pipeline_clear_keys(ctx9, co, rks):
    """no fips: the reference-order cipher at 14 rounds, ctr_mode.ref_block_fn its byte model"""
    from ctr_mode import ref_block_fn
    from pipeline import AESPipeline
    p = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)
    pt = np.random.default_rng(0x256).integers(0, 256, 16).astype(np.uint8)
    ct = p.encrypt(pt, rks[32])
    assert np.array_equal(p.encoder.decode(*ct), ref_block_fn(rks[32])(pt))
    assert np.array_equal(p.encoder.decode(*p.decrypt(*ct, rks[32])), pt)


def test_two_states_two_keys(ctx9, co):
    from aes_keyschedule import expand_aes_key
    from ctr_mode import ctr_xor, fips_block_fn
    from pipeline import AESPipeline
    pipe2 = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=2, fips=True)
    rng = np.random.default_rng(0x2E6)
    keys = rng.integers(0, 256, (2, 32)).astype(np.uint8)
    clear = [expand_aes_key(k) for k in keys]
    erk, _ = _expand(pipe2, keys)
    for r in (2, 3, 14):
        assert np.array_equal(pipe2.encoder.decode(*erk[r]), np.stack([c[r] for c in clear])), r
    nonce, c0 = bytes(range(0xB0, 0xBC)), 2 ** 32 - 1  # the second state's counter wraps to 0
    m = rng.integers(0, 256, (2, 16)).astype(np.uint8)
    # state b holds block b of the stream under ITS key: row b of the two-block CTR encryption with key b
    c = np.stack([ctr_xor(fips_block_fn(clear[b]), m, nonce, c0)[b] for b in (0, 1)])
    assert np.array_equal(pipe2.encoder.decode(*pipe2.transcipher(c, nonce, c0, erk)), m)
    vals = pipe2.encoder.decode_values(pipe2.transcipher_values(c, nonce, c0, erk)) * 256.0
    print(f"AES-256 transcipher_values, two states: max value error {np.abs(vals - m).max():.3g} byte units")
    assert np.array_equal(np.rint(vals), m)


def test_aes192_clear_and_client_encoded_keys(pipe, rks):
    from key_expansion import EncryptedRoundKeys
    assert len(rks[24]) == 13
    assert bytes(pipe.encoder.decode(*pipe.encrypt(_u8(PT), rks[24]))).hex() == C2_CT
    erk = EncryptedRoundKeys.from_pairs([pipe.encoder.encode(k) for k in rks[24]], pipe.layout)
    ct = pipe.encrypt(_u8(PT), erk)
    assert bytes(pipe.encoder.decode(*ct)).hex() == C2_CT
    assert len(erk.packed) == 13 and all(k is not None for k in erk.packed[1:12])
    assert np.array_equal(pipe.encoder.decode(*pipe.decrypt(*ct, erk)), _u8(PT))


def test_no_cache_leaks_across_schedules(ctx9, co, rks):
    """one pipeline, schedules of different lengths in turn: 256 then 128, and 128 then 256 (then 192)"""
    from pipeline import AESPipeline
    p = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True)
    enc = lambda n: bytes(p.encoder.decode(*p.encrypt(_u8(PT), rks[n]))).hex()
    assert enc(32) == C3_CT
    assert enc(16) == C1_CT           # after an AES-256 call
    assert enc(32) == C3_CT           # and the other order
    assert enc(24) == C2_CT
    assert enc(16) == C1_CT
    ct = p.encrypt(_u8(PT), rks[32])
    p.encrypt(_u8(PT), rks[16])
    assert np.array_equal(p.encoder.decode(*p.decrypt(*ct, rks[32])), _u8(PT))


def test_seeded_key_crosses_the_wire(pipe, rks):
    from state_encoder import dump_ct_seeded, load_ct_seeded
    ck = pipe.encrypt_key(KEY32, seeded=True)
    assert len(ck) == 4
    ids = [c.seed_id >> 16 for c in ck]
    assert ids == list(range(ids[0], ids[0] + 4))   # one batched seeded encryption made all four
    wire = [dump_ct_seeded(pipe.ctx, c) for c in ck]
    back = [load_ct_seeded(pipe.ctx, b, level, sid, tag) for b, level, tag, sid in wire]
    erk = pipe.expand_key(*back)
    assert len(erk) == 15 and np.array_equal(pipe.encoder.decode(*erk[14]), rks[32][14])


class _NoSecretKeyRenorm:
    """the context with every secret-key renorm entry made to raise (tests/test_gpu_key_expansion.py): true-FHE mode
    may only refresh by bootstrap + snap"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        if name.startswith("renorm"):
            def refuse(*a, **k):
                raise AssertionError(f"true-FHE path called the secret-key renorm {name}")
            return refuse
        return getattr(self._ctx, name)


def test_true_fhe_expand_then_encrypt(co):
    """the 11 / 4 true-FHE set of tests/test_gpu_key_expansion.py: the 32-byte key is expanded and used with
    bootstrap + snap as the only renorm"""
    import mi355x_ckks
    from engine_context import EngineContext
    from pipeline import AESPipeline
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    fhe = AESPipeline(_NoSecretKeyRenorm(c12), co, use_hard_renorm_between_steps=False, true_fhe=True, fips=True)
    assert fhe.encoder.renorm_hook is not None
    ck = fhe.encrypt_key(KEY32)
    c12.engine.sync()
    n0, b0, t0 = mi355x_ckks.launch_count(), c12.bootstrap_stats()["calls"], time.perf_counter()
    erk = fhe.expand_key(*ck)
    c12.engine.sync()
    print(f"AES-256 expand_key true_fhe: {time.perf_counter() - t0:.3f} s, {mi355x_ckks.launch_count() - n0} launches, "
          f"{c12.bootstrap_stats()['calls'] - b0} bootstrap calls")
    b1, t1 = c12.bootstrap_stats()["calls"], time.perf_counter()
    ct = fhe.encrypt(_u8(PT), erk)
    c12.engine.sync()
    print(f"AES-256 encrypt true_fhe: {time.perf_counter() - t1:.3f} s, {c12.bootstrap_stats()['calls'] - b1} bootstrap calls")
    assert bytes(fhe.encoder.decode(*ct)).hex() == C3_CT


def test_evaluation_only_server_expands_the_key(co, rks):
    """client and server of tests/test_gpu_eval_context.py::test_transcipher_end_to_end_with_no_secret_on_the_server (the
    11 / 4 set): the client's warm-up runs the 256-bit expand_key, so the exported bundle carries the word copy's
    rotation keys; the server, which holds no secret, expands the client's encrypted key; the client decodes key 14"""
    from engine_context import EngineContext
    from pipeline import AESPipeline
    from state_encoder import dump_ct, load_ct
    client = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xE2E, enc_nonce=0xE2E)
    cpipe = AESPipeline(client, co, true_fhe=True, fips=True)
    warm_key = np.random.default_rng(0xE2E).integers(0, 256, 32).astype(np.uint8)
    before = set(client.engine.key_ids())
    cpipe.expand_key(*cpipe.encrypt_key(warm_key))        # the warm-up: every key the expansion touches now exists
    made = set(client.engine.key_ids()) - before
    server = EngineContext.from_evaluation_keys(client.export_evaluation_keys(stream=True))
    assert server.secret_key is None and not server.engine.has_secret
    assert made <= set(server.engine.key_ids())
    print(f"evaluation-only: the 256-bit expansion's warm-up made {len(made)} switching keys, the bundle holds {len(server.engine.key_ids())}")
    spipe = AESPipeline(server, co, true_fhe=True, fips=True)
    wire = [dump_ct(client, c) for c in cpipe.encrypt_key(KEY32)]
    serk = spipe.expand_key(*(load_ct(server, *w) for w in wire))
    back = [load_ct(client, *dump_ct(server, c)) for c in serk[14]]
    assert np.array_equal(cpipe.encoder.decode(*back), rks[32][14])


def test_refusals(pipe, ctx9, co, expanded):
    from pipeline import AESPipeline
    erk, _ = expanded
    with pytest.raises(ValueError, match="AES-192"):
        pipe.encrypt_key(KEY24)
    pairs2 = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, pairs=2, fips=False)
    plain = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)
    from key_expansion import EncryptedRoundKeys
    from aes_keyschedule import expand_aes_key
    plain_keys = EncryptedRoundKeys.from_pairs([plain.encoder.encode(k) for k in expand_aes_key(KEY32)], plain.layout)
    with pytest.raises(ValueError, match="pairs"):
        pairs2.encrypt(np.zeros((2, 16), np.uint8), plain_keys)
    with pytest.raises(ValueError, match="transposed"):
        plain.expand_key(*pipe.encrypt_key(KEY32))     # a 4-tuple built for the FIPS byte order
    with pytest.raises(ValueError, match="transposed"):
        plain.encrypt(_u8(PT), erk)
    with pytest.raises(ValueError):
        pipe.expand_key(*pipe.encrypt_key(KEY32)[:3])  # half a second pair
    with pytest.raises(ValueError, match="11 round keys"):
        pipe.encrypt(_u8(PT), expand_aes_key(KEY32)[:12])
