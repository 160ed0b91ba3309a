"""AESPipeline(fips=True): FIPS-197 AES-128 on the C2 set of tests/test_gpu_ctr.py (boot_fresh_level=7, dnum=4).

The pipeline's round sequence with ShiftColumns in place of ShiftRows on byte-transposed states (pipeline.py,
shift_columns.py); the references are oracle/aes_plain.fips_encrypt, FIPS-197 Appendix C.1 and NIST SP 800-38A
F.5.1.  Measured on an MI355X: the FIPS encrypt output's largest slot error is 2.27e-5 rad, 8642x inside the
decode margin pi / 16 (the test asks 100x, as tests/test_gpu_ctr.py does)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C1_KEY = bytes(range(16))
C1_PT = bytes.fromhex("00112233445566778899aabbccddeeff")
C1_CT = "69c4e0d86a7b0430d8cdb78070b4c55a"


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
    return expand_aes128_key(np.frombuffer(C1_KEY, np.uint8))


@pytest.fixture(scope="module")
def pipe(ctx9, co):
    from pipeline import AESPipeline
    return AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True)


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


def test_encrypt_decrypt_fips(pipe, ctx9, rks):
    from oracle import aes_plain
    from shift_columns import transpose_bytes
    from utils import ZetaEncoder
    assert pipe.packed_xor and pipe._sr_entry_ok()  # the headline path: ShiftColumns inside MixColumns' packed entry
    dbg = {}
    ct = pipe.encrypt(_u8(C1_PT), rks, debug=dbg)
    got = pipe.encoder.decode(*ct)
    assert bytes(got).hex() == C1_CT
    assert np.array_equal(dbg["enc.r0.ark"]["plain"], _u8(C1_PT) ^ rks[0])  # snapshots decode to FIPS byte order
    assert np.array_equal(dbg["enc.r1.sr"]["plain"], aes_plain.shift_rows(aes_plain.SBOX[_u8(C1_PT) ^ rks[0]]))
    # precision: the held state is T(ciphertext); the largest slot error against its codewords
    held = transpose_bytes(got)[None, :]
    err = 0.0
    for c, want in zip(ct, (held >> 4, held & 15)):
        z = pipe.encoder._take(ctx9.decrypt(c))
        err = max(err, float(np.abs(np.angle(z / ZetaEncoder.to_zeta(want, 16))).max()))
    margin = (np.pi / 16) / err
    print(f"fips encrypt: max slot error {err:.3g} rad, margin {margin:.0f}x inside pi/16")
    assert margin >= 100.0
    assert np.array_equal(pipe.encoder.decode(*pipe.decrypt(*ct, rks)), _u8(C1_PT))
    p = np.random.default_rng(0xF1).integers(0, 256, 16).astype(np.uint8)
    ct = pipe.encrypt(p, rks)
    assert np.array_equal(pipe.encoder.decode(*ct), aes_plain.fips_encrypt(p, rks))
    assert np.array_equal(pipe.encoder.decode(*pipe.decrypt(*ct, rks)), p)


def test_shift_columns_and_entry_decode_to_the_byte_model(pipe):
    """on FIPS-ordered bytes ShiftColumns of the held T(state) reads as ShiftRows; the entry's second output is
    that state shifted by one column of the held order"""
    from oracle import aes_plain
    from shift_columns import shift_columns_bytes, transpose_bytes
    enc = pipe.encoder
    s = np.random.default_rng(5).integers(0, 256, 16).astype(np.uint8)
    assert np.array_equal(enc.decode(*pipe.shift.apply(*enc.encode(s))), aes_plain.shift_rows(s))
    assert np.array_equal(enc.decode(*pipe.invshift.apply(*enc.encode(s))), aes_plain.inv_shift_rows(s))
    p0, p1 = pipe.mix.sr_entry(*enc.encode(s), pipe.shift)
    held = shift_columns_bytes(transpose_bytes(s), -1)
    assert np.array_equal(enc.decode_packed(p0), transpose_bytes(held))
    assert np.array_equal(enc.decode_packed(p0), aes_plain.shift_rows(s))
    assert np.array_equal(enc.decode_packed(p1), transpose_bytes(held[(np.arange(16) + 4) % 16]))


def test_transcipher_two_states(ctx9, co, rks):
    from ctr_mode import ctr_xor, fips_block_fn
    from oracle import aes_plain
    from pipeline import AESPipeline
    pipe2 = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, states=2, fips=True)
    assert pipe2.layout.periodic
    nonce = bytes(range(0xA0, 0xAC))
    m = np.random.default_rng(6).integers(0, 256, (2, 16)).astype(np.uint8)
    c = ctr_xor(lambda b: aes_plain.fips_encrypt(b, rks), m, nonce, 2 ** 32 - 1)  # the second counter wraps to 0
    assert np.array_equal(c, ctr_xor(fips_block_fn(rks), m, nonce, 2 ** 32 - 1))
    assert np.array_equal(pipe2.encoder.decode(*pipe2.transcipher(c, nonce, 2 ** 32 - 1, rks)), m)


def test_sp800_38a_f51_keystream_block1(pipe):
    """CTR-AES128.Encrypt block 1: the 16-byte initial counter block passed as nonce12 plus counter"""
    from aes_keyschedule import expand_aes128_key
    key = expand_aes128_key(_u8(bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")))
    icb = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
    pt1, ct1 = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a"), bytes.fromhex("874d6191b620e3261bef6864990db6ce")
    ks = pipe.encoder.decode(*pipe.ctr_keystream(icb[:12], int.from_bytes(icb[12:], "big"), key))
    assert bytes(ks).hex() == bytes(a ^ b for a, b in zip(pt1, ct1)).hex() == "ec8cdf7398607cb0f2d21675ea9ea1e4"


def test_plain_pipeline_refuses_a_fips_pair(pipe, ctx9, co, rks):
    from pipeline import AESPipeline
    plain = AESPipeline(ctx9, co, use_hard_renorm_between_steps=True)
    ct = pipe.encoder.encode(_u8(C1_PT))
    with pytest.raises(ValueError, match="transposed"):
        plain.decrypt(*ct, rks)
    with pytest.raises(ValueError, match="transposed"):
        plain.encoder.decode(*ct)
    with pytest.raises(ValueError):
        pipe.decrypt(*plain.encoder.encode(_u8(C1_PT)), rks)
    for kw in ({"fuse_sub_ark": True}, {"fuse_sr_mc": True}, {"pairs": 2}):
        with pytest.raises(ValueError, match="fips"):
            AESPipeline(ctx9, co, use_hard_renorm_between_steps=True, fips=True, **kw)


def test_true_fhe_encrypt_fips(co, rks):
    """the 11 / 4 true-FHE set of tests/test_gpu_ctr.py: bootstrap + snap the only renorm, FIPS-197 bytes out"""
    from engine_context import EngineContext
    from pipeline import AESPipeline
    c12 = EngineContext(signature=1, boot_fresh_level=11, dnum=4, thread_count=4, seed=0xF12, enc_nonce=0xF12)
    fhe = AESPipeline(c12, co, use_hard_renorm_between_steps=False, true_fhe=True, fips=True)
    assert fhe.encoder.renorm_hook is not None
    assert bytes(fhe.encoder.decode(*fhe.encrypt(_u8(C1_PT), rks))).hex() == C1_CT
