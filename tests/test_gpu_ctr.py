"""AES-CTR transciphering (AESPipeline.encrypt_public / ctr_keystream / transcipher, ctr_mode.py) on the C2 set.

The block function is the pipeline's own cipher (oracle/aes_plain.ref_encrypt), not FIPS-197:
the byte model is ctr_mode.ctr_xor over ref_encrypt, and the NIST SP 800-38A vectors do not apply."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONCE = bytes(range(0xA0, 0xAC))


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
    return expand_aes128_key(np.random.default_rng(0xC7).integers(0, 256, 16).astype(np.uint8))


@pytest.fixture(scope="module")
def pipe1(ctx9, co):
    from pipeline import AESPipeline
    return AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)


def _block_fn(rks):
    from oracle import aes_plain
    return lambda blk: aes_plain.ref_encrypt(blk, rks)


def test_encrypt_public_matches_encrypt(pipe1, rks):
    from oracle import aes_plain
    rng = np.random.default_rng(41)
    for _ in range(2):
        pt = rng.integers(0, 256, 16).astype(np.uint8)
        dbg = {}
        ct = pipe1.encrypt_public(pt, rks, debug=dbg)
        assert np.array_equal(pipe1.encoder.decode(*ct), aes_plain.ref_encrypt(pt, rks))
        assert dbg and "enc.input" not in dbg and "enc.r0.ark" in dbg and "enc.output" in dbg
        assert all(v["plain"] is not None for v in dbg.values())
        assert np.array_equal(dbg["enc.r0.ark"]["plain"], pt ^ rks[0])
    assert ct[0].level == pipe1.encrypt(pt, rks)[0].level


def test_transcipher_one_state_and_counter_wrap(pipe1, rks):
    from ctr_mode import ctr_xor
    rng = np.random.default_rng(42)
    fn = _block_fn(rks)
    out_level = None
    for counter0 in (2 ** 32 - 1, 0):  # the block after counter 2^32 - 1 is counter 0: the second call is the wrap
        m = rng.integers(0, 256, (1, 16)).astype(np.uint8)
        ks = ctr_xor(fn, np.zeros((1, 16), np.uint8), NONCE, counter0)
        assert np.array_equal(pipe1.encoder.decode(*pipe1.ctr_keystream(NONCE, counter0, rks)), ks[0])
        ct = pipe1.transcipher((m ^ ks)[0], NONCE, counter0, rks)
        assert np.array_equal(pipe1.encoder.decode(*ct), m[0])
        out_level = ct[0].level
    two = ctr_xor(fn, np.zeros((2, 16), np.uint8), NONCE, 2 ** 32 - 1)
    assert np.array_equal(two[1], ks[0])  # the byte model's own wrap agrees with the second call's counter
    assert out_level == pipe1.encrypt(m[0], rks)[0].level


def test_transcipher_64_states_periodic(ctx9, co, rks):
    """64 consecutive counters in one ciphertext pair (periodic layout), every state checked; the largest slot
    error of the output stays inside the decode margin pi/16 by at least the 100x asked of true-FHE runs"""
    from ctr_mode import ctr_xor
    from pipeline import AESPipeline
    from utils import ZetaEncoder
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=64)
    assert pipe.layout.periodic
    rng = np.random.default_rng(43)
    m = rng.integers(0, 256, (64, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 2 ** 32 - 40)  # the 64 counters cross the wrap
    hi, lo = pipe.transcipher(c, NONCE, 2 ** 32 - 40, rks)
    got = pipe.encoder.decode(hi, lo)
    bad = [j for j in range(64) if not np.array_equal(got[j], m[j])]
    assert not bad, bad[:8]
    err = 0.0
    for ct, want in ((hi, m >> 4), (lo, m & 15)):
        z = pipe.encoder._take(ctx9.decrypt(ct))
        err = max(err, float(np.abs(np.angle(z / ZetaEncoder.to_zeta(want, 16))).max()))
    margin = (np.pi / 16) / err
    print(f"transcipher, 64 states: max slot error {err:.3g} rad, margin {margin:.0f}x inside pi/16")
    assert margin >= 100.0


def test_transcipher_true_fhe(co, rks, monkeypatch):
    """the 11 / 4 true-FHE set: one block, the bootstrap + snap hook the only renorm (no secret-key call between
    the key's encryption and the output)"""
    from ctr_mode import ctr_xor
    from engine_context import EngineContext
    from pipeline import AESPipeline
    from test_gpu_true_fhe import _no_secret_renorm
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    pipe = AESPipeline(c12, co, use_hard_renorm_between_steps=False, true_fhe=True)
    assert pipe.encoder.renorm_hook is not None
    m = np.random.default_rng(44).integers(0, 256, (1, 16)).astype(np.uint8)
    c = ctr_xor(_block_fn(rks), m, NONCE, 7)
    pipe._prepare_round_keys(rks)  # the key's encryption is the client's part
    _no_secret_renorm(c12, monkeypatch)
    b0 = c12.bootstrap_stats()["count"]
    ct = pipe.transcipher(c[0], NONCE, 7, rks)
    n_boot = c12.bootstrap_stats()["count"] - b0
    monkeypatch.undo()
    assert np.array_equal(pipe.encoder.decode(*ct), m[0])
    print(f"true-FHE transcipher: {n_boot} ciphertexts bootstrapped")
    assert n_boot > 0
    assert ct[0].level == pipe.encrypt(m[0], rks)[0].level


def test_pairs_refused(ctx9, co, rks):
    from pipeline import AESPipeline
    pipe = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, pairs=2)
    blk = np.zeros(16, np.uint8)
    with pytest.raises(ValueError):
        pipe.encrypt_public(blk, rks)
    with pytest.raises(ValueError):
        pipe.ctr_keystream(NONCE, 0, rks)
    with pytest.raises(ValueError):
        pipe.transcipher(blk, NONCE, 0, rks)
