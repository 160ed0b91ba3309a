"""AESPipeline.expand_key / EncryptedRoundKeys (key_expansion.py) on the C2 set of tests/test_gpu_fips.py
(boot_fresh_level=7, dnum=4): the 11 AES-128 round keys derived homomorphically from ONE encrypted key, then used by
encrypt / decrypt / transcipher in place of clear round keys.

References: aes_keyschedule.expand_aes128_key, key_expansion.schedule_step_bytes for the debug stages, FIPS-197
Appendix C.1, ctr_mode.ctr_xor(fips_block_fn(...)).  Precision: the largest slot error of any expanded key must sit at
least 100x inside the decode margin pi / 16, the margin tests/test_gpu_ctr.py and tests/test_gpu_fips.py ask of
their outputs.  Every test prints what it measures (time, launches, renorms, margin); DESIGN.md §3.19 records them.
Measured on an MI355X: largest slot error of any expanded key 3.53e-5 rad with fips=True (5565x inside pi / 16),
5.14e-5 rad in the default pipeline (3822x)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C1_KEY = bytes(range(16))
C1_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
C1_CT = "69c4e0d86a7b0430d8cdb78070b4c55a"


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


@pytest.fixture(scope="module")
def ctx9():
    from engine_context import EngineContext
    return EngineContext(signature=1, boot_fresh_level=7, dnum=4, thread_count=4, seed=0xC2C2, enc_nonce=0xC2C2)


@pytest.fixture(scope="module")
def co(coeff_dir):
    from aes_keyschedule import load_all_coeffs
    return load_all_coeffs(coeff_dir)


@pytest.fixture(scope="module")
def rks():
    from aes_keyschedule import expand_aes128_key
    return expand_aes128_key(_u8(C1_KEY))


@pytest.fixture(scope="module")
def pipe(ctx9, co):
    from pipeline import AESPipeline
    return AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True)


def _expand(p, key):
    """(EncryptedRoundKeys, debug stages) with the expansion's time, launches and renorms printed"""
    import mi355x_ckks
    from utils import RENORM_TALLY
    ck = p.encrypt_key(key)
    p.ctx.engine.sync()
    dbg = {}
    n0, r0, t0 = mi355x_ckks.launch_count(), RENORM_TALLY["calls"], time.perf_counter()
    erk = p.expand_key(*ck, debug=dbg)
    p.ctx.engine.sync()
    dt = time.perf_counter() - t0
    print(f"expand_key fips {int(p.fips)} true_fhe {int(p.true_fhe)} states {p.states} (with debug decodes): {dt:.3f} s, "
          f"{mi355x_ckks.launch_count() - n0} launches, {RENORM_TALLY['calls'] - r0} secret-key renorm calls, "
          f"{p.ctx.bootstrap_stats()['calls'] if hasattr(p.ctx, 'bootstrap_stats') else 0} bootstrap calls so far")
    return erk, dbg


@pytest.fixture(scope="module")
def expanded(pipe):
    return _expand(pipe, _u8(C1_KEY))


def _check_expansion(p, erk, dbg, rks):
    from key_expansion import EncryptedRoundKeys, schedule_step_bytes
    from utils import ZetaEncoder
    assert isinstance(erk, EncryptedRoundKeys) and len(erk) == 11
    enc = p.encoder
    err, fresh = 0.0, enc.encode(rks[0])[0].level
    for r in range(11):
        got = enc.decode(*erk[r])
        assert np.array_equal(got, rks[r]), (r, bytes(got).hex(), bytes(rks[r]).hex())
        assert erk[r][0].level == erk[r][1].level == fresh  # the level _encode_key hands out
        held = enc._order(got[None, :])
        for c, want in zip(erk[r], (held >> 4, held & 15)):
            z = enc._take(p.ctx.decrypt(c))
            err = max(err, float(np.abs(np.angle(z / ZetaEncoder.to_zeta(want, 16))).max()))
    want = schedule_step_bytes(rks[0], 1)
    for name in ("prefix", "sub", "rot", "out"):
        assert np.array_equal(dbg[f"ks.r1.{name}"]["plain"], want[name]), name
    assert set(dbg) == {f"ks.r{r}.{s}" for r in range(1, 11) for s in ("prefix", "sub", "rot", "out")}
    margin = (np.pi / 16) / err
    print(f"expanded keys fips {int(p.fips)}: max slot error {err:.3g} rad, margin {margin:.0f}x inside pi/16")
    assert margin >= 100.0


def test_expansion_fips(pipe, expanded, rks):
    _check_expansion(pipe, *expanded, rks)


def test_expansion_default_pipeline(ctx9, co, rks):
    from pipeline import AESPipeline
    p = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)
    _check_expansion(p, *_expand(p, _u8(C1_KEY)), rks)


def test_fips_encrypt_decrypt_with_expanded_keys(pipe, expanded):
    erk, _ = expanded
    ct = pipe.encrypt(_u8(C1_PT), erk)
    assert bytes(pipe.encoder.decode(*ct)).hex() == C1_CT
    assert all(k is not None for k in erk.packed[1:10]) and erk.packed[0] is None  # packed homomorphically, kept on the keys
    assert np.array_equal(pipe.encoder.decode(*pipe.decrypt(*ct, erk)), _u8(C1_PT))


def test_transcipher_two_states_two_keys(ctx9, co):
    from aes_keyschedule import expand_aes128_key
    from ctr_mode import ctr_xor, fips_block_fn
    from pipeline import AESPipeline
    pipe2 = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=2, fips=True)
    rng = np.random.default_rng(0x2E)
    keys = rng.integers(0, 256, (2, 16)).astype(np.uint8)
    erk, _ = _expand(pipe2, keys)
    for r in (1, 10):
        assert np.array_equal(pipe2.encoder.decode(*erk[r]), np.stack([expand_aes128_key(k)[r] for k in keys]))
    nonce, c0 = bytes(range(0xB0, 0xBC)), 2 ** 32 - 1  # the second state's counter wraps to 0
    m = rng.integers(0, 256, (2, 16)).astype(np.uint8)
    # state b holds block b of the stream under ITS key: row b of the two-block CTR encryption with key b
    c = np.stack([ctr_xor(fips_block_fn(expand_aes128_key(keys[b])), m, nonce, c0)[b] for b in (0, 1)])
    assert np.array_equal(pipe2.encoder.decode(*pipe2.transcipher(c, nonce, c0, erk)), m)


def test_from_pairs_gives_the_bytes_of_clear_round_keys(pipe, rks):
    from key_expansion import EncryptedRoundKeys
    erk = EncryptedRoundKeys.from_pairs([pipe.encoder.encode(k) for k in rks], pipe.layout)
    p = np.random.default_rng(0xF7).integers(0, 256, 16).astype(np.uint8)
    clear = pipe.encoder.decode(*pipe.encrypt(p, rks))
    assert np.array_equal(pipe.encoder.decode(*pipe.encrypt(p, erk)), clear)
    assert np.array_equal(pipe.encoder.decode(*pipe.encrypt(p, rks)), clear)  # and clear keys behave as before, after


def test_refusals(pipe, ctx9, co, rks):
    from key_expansion import EncryptedRoundKeys
    from pipeline import AESPipeline
    fips_keys = EncryptedRoundKeys.from_pairs([pipe.encoder.encode(k) for k in rks], pipe.layout)
    plain = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)
    with pytest.raises(ValueError, match="transposed"):
        plain.encrypt(_u8(C1_PT), fips_keys)
    with pytest.raises(ValueError, match="transposed"):
        plain.expand_key(*pipe.encrypt_key(_u8(C1_KEY)))
    with pytest.raises(ValueError, match="transposed"):
        EncryptedRoundKeys.from_pairs(fips_keys.pairs, plain.layout)
    two = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=2)
    with pytest.raises(ValueError):
        two.decrypt(*two.encoder.encode(np.zeros((2, 16), np.uint8)), fips_keys)
    plain_keys = EncryptedRoundKeys.from_pairs([plain.encoder.encode(k) for k in rks], plain.layout)
    pairs2 = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, pairs=2)
    with pytest.raises(ValueError, match="pairs"):
        pairs2.encrypt(np.zeros((2, 16), np.uint8), plain_keys)
    with pytest.raises(ValueError, match="pairs"):
        pairs2.expand_key(*plain.encrypt_key(_u8(C1_KEY)))
    fused = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fuse_sub_ark=True)
    with pytest.raises(ValueError, match="fuse_sub_ark"):
        fused.encrypt(_u8(C1_PT), plain_keys)
    with pytest.raises(ValueError, match="11 round keys"):
        EncryptedRoundKeys.from_pairs(plain_keys.pairs[:10], plain.layout)


class _NoSecretKeyRenorm:
    """the context with every secret-key renorm entry made to raise (as tests/test_gpu_packed_xor.py's _NoFolds
    does for the folding ones): true-FHE mode may only refresh by bootstrap + snap"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        if name.startswith("renorm"):
            def refuse(*a, **k):
                raise AssertionError(f"true-FHE path called the secret-key renorm {name}")
            return refuse
        return getattr(self._ctx, name)


def test_true_fhe_expand_then_encrypt(co):
    """the 11 / 4 true-FHE set of tests/test_gpu_fips.py: the key is expanded and used with bootstrap + snap as the
    only renorm, nothing on the server in clear but public data"""
    from engine_context import EngineContext
    from pipeline import AESPipeline
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    fhe = AESPipeline(_NoSecretKeyRenorm(c12), co, use_hard_renorm_between_steps=False, true_fhe=True, fips=True)
    assert fhe.encoder.renorm_hook is not None
    import mi355x_ckks
    ck = fhe.encrypt_key(_u8(C1_KEY))
    c12.engine.sync()
    n0, b0, t0 = mi355x_ckks.launch_count(), c12.bootstrap_stats()["calls"], time.perf_counter()
    erk = fhe.expand_key(*ck)
    c12.engine.sync()
    print(f"expand_key true_fhe: {time.perf_counter() - t0:.3f} s, {mi355x_ckks.launch_count() - n0} launches, "
          f"{c12.bootstrap_stats()['calls'] - b0} bootstrap calls")
    assert bytes(fhe.encoder.decode(*fhe.encrypt(_u8(C1_PT), erk))).hex() == C1_CT
