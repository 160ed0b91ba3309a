"""The client side of ring-switched result packs (result_pack.py), numpy only: a small-ring ciphertext
made here decrypts to the members; the small ring's slots are the big ring's; the security table; the choice of the ring
against stub contexts; the meta through json; every ValueError."""
import json

import numpy as np
import pytest

import result_pack as rp

Q = (1073479681, 1073184769)          # two 30-bit primes (any two coprime moduli do: the client side uses no transform)
SCALE = float(2 ** 40)


def _big_slots(coeffs_big):
    """slot t = p(zeta^(5^t)), zeta = exp(i pi / N), by direct evaluation on the nonzero coefficients"""
    n = coeffs_big.shape[0]
    e = rp.slot_exponents(n // 2)
    nz = np.flatnonzero(coeffs_big)
    ang = np.pi * ((e[:, None] * nz[None, :]) % (2 * n)) / n
    return (coeffs_big[nz][None, :] * np.exp(1j * ang)).sum(axis=1)


def _message_coeffs(members, period, ring, sc_small):
    """integer coefficients (scale SCALE) of the packed message in the ring of degree `ring`: the inverse of
    small_ring_slots on a conjugate-symmetric completion, rounded"""
    z = rp.pack_slots(members, period, sc_small)
    r = ring
    e = rp.slot_exponents(r // 2)
    ev = np.zeros(r, np.complex128)                    # ev[m] = p(w^(2 m + 1))
    idx = ((e % (2 * r)) - 1) // 2
    ev[idx] = z
    ev[(r - 1 - idx) % r] = np.conj(z)                 # w^-(2 m + 1) = w^(2 (R - 1 - m) + 1)
    c = np.fft.fft(ev / r) * np.exp(-1j * np.pi * np.arange(r) / r)
    assert np.abs(c.imag).max() < 1e-9
    return np.rint(c.real * SCALE).astype(np.int64)


def _encrypt(rng, msg, ring):
    """(array (2, 2, R), s_R): c1 uniform, c0 = m - c1 s_R per limb, exact negacyclic products"""
    s = rng.integers(-1, 2, ring)
    arr = np.zeros((2, 2, ring), np.uint32)
    for l, q in enumerate(Q):
        c1 = rng.integers(0, q, ring)
        prod = np.zeros(ring, dtype=object)
        for i in np.flatnonzero(s):
            sh = np.concatenate((-c1[ring - i:], c1[:ring - i])) if i else c1
            prod = prod + int(s[i]) * sh.astype(object)
        arr[0, l] = np.array([(int(m) - int(p)) % q for m, p in zip(msg, prod)], np.uint32)
        arr[1, l] = c1
    return arr, s.astype(np.int32)


@pytest.mark.parametrize("ring", [512, 2048])
@pytest.mark.parametrize("G,period", [(1, 16), (4, 16), (2, 64)])
def test_a_numpy_ciphertext_decrypts_to_the_members(ring, G, period):
    """ternary s_R, two 30-bit primes, a message in the subring: ring_decrypt -> slots -> split_slots returns the members
    to 1e-9.  The phase is exact; the one error is the rounding of the message's coefficients to integers, at most
    R / 2 / scale per slot, 9.4e-10 at R = 2048 and the scale 2^40 used here (|coefficients| < 2^41 < q0 q1 / 2)"""
    rng = np.random.default_rng(11 * ring + G + period)
    sc_big = 4096                                      # the big ring's slot count the client tiles to
    members = [rng.uniform(-1, 1, period) + 1j * rng.uniform(-1, 1, period) for _ in range(G)]
    msg = _message_coeffs(members, period, ring, ring // 2)
    arr, s = _encrypt(rng, msg, ring)
    assert np.count_nonzero(s) > ring // 2
    z = rp.ring_decrypt(arr, s, dict(ring=ring, slots=sc_big, moduli=list(Q), scale=SCALE))
    assert z.shape == (sc_big,)
    back = rp.split_slots(z, G, period)
    for j in range(G):
        assert back[j].shape == (sc_big,)
        assert np.abs(back[j] - np.tile(members[j], sc_big // period)).max() <= 1e-9, j


@pytest.mark.parametrize("ring,n", [(512, 4096), (2048, 8192), (16, 64)])
def test_decimated_big_ring_slots_equal_small_ring_slots(ring, n):
    rng = np.random.default_rng(ring)
    k = n // ring
    small = rng.integers(-1000, 1000, ring).astype(np.float64)
    big = np.zeros(n)
    big[::k] = small
    want = _big_slots(big)                             # n / 2 slots of the big ring
    got = rp.small_ring_slots(small)
    assert got.shape == (ring // 2,)
    assert np.abs(np.tile(got, (n // 2) // (ring // 2)) - want).max() <= 1e-9 * np.abs(want).max()


def test_max_log_modulus_is_the_table():
    assert [rp.max_log_modulus(r) for r in (1024, 2048, 4096, 8192, 16384, 32768)] == [27, 54, 109, 218, 438, 881]
    assert rp.max_log_modulus(512) == 0 and rp.max_log_modulus(3000) == 0 and rp.max_log_modulus(0) == 0


class _Engine:
    def __init__(self, log_n, n_p=3, special_bits=30):
        self.n = 1 << log_n
        self.slot_count = self.n // 2
        self.n_q = 4
        sp = [1073479681 - 2 * i if special_bits == 30 else (1 << special_bits) - 1 for i in range(n_p)]
        self._mod = [1073741441, 1073740609, 999999937, 1073479999] + sp

    def moduli(self):
        return np.array(self._mod, np.uint32)


def test_auto_takes_the_smallest_accepted_ring():
    e16 = _Engine(16)
    assert rp._choose_ring(e16, 8, 256, "auto", False) == 4096           # 2 G P = 4096: 90 bits <= 109
    assert rp._choose_ring(e16, 1, 16, "auto", False) == 4096            # 32 coefficients, but 2048 admits 54 bits only
    assert rp._choose_ring(e16, 32, 256, "auto", False) == 16384
    assert rp._choose_ring(e16, 1, 16, "auto", True) == 32               # insecure_ok: the smallest that fits
    assert rp._choose_ring(_Engine(16, special_bits=20), 1, 16, "auto", False) == 4096   # 80 bits: still above 54
    assert rp._choose_ring(e16, 8, 256, 8192, False) == 8192
    with pytest.raises(ValueError, match="no ring below N"):
        rp._choose_ring(_Engine(12), 1, 16, "auto", False)               # N = 4096: nothing below it is accepted
    with pytest.raises(ValueError, match="no ring below N"):
        rp._choose_ring(_Engine(13), 32, 128, "auto", True)              # 2 G P = N


def test_every_value_error():
    e = _Engine(13)
    for ring in (0, -4, 3, 1000, 8192, 16384, "smallest"):
        with pytest.raises(ValueError):
            rp._choose_ring(e, 1, 16, ring, True)
    with pytest.raises(ValueError, match="do not fit"):
        rp._choose_ring(e, 8, 64, 512, True)
    with pytest.raises(ValueError, match="ring too small for this modulus"):
        rp._choose_ring(e, 1, 16, 512, False)
    with pytest.raises(ValueError, match="ring too small for this modulus"):
        rp._choose_ring(e, 1, 16, 2048, False)
    assert rp._choose_ring(e, 1, 16, 4096, False) == 4096
    arr = np.zeros((2, 2, 512), np.uint32)
    s = np.zeros(512, np.int32)
    meta = dict(ring=512, slots=4096, moduli=list(Q), scale=SCALE)
    assert np.abs(rp.ring_decrypt(arr, s, meta)).max() == 0
    with pytest.raises(ValueError, match="array"):
        rp.ring_decrypt(arr[:, :, :256], s, meta)
    with pytest.raises(ValueError, match="array"):
        rp.ring_decrypt(np.zeros((2, 2, 4096), np.uint32), s, meta)
    with pytest.raises(ValueError, match="ternary"):
        rp.ring_decrypt(arr, s[:100], meta)
    with pytest.raises(ValueError, match="ternary"):
        rp.ring_decrypt(arr, s + 2, meta)
    bad = arr.copy()
    bad[1, 1, 5] = Q[1]
    with pytest.raises(ValueError, match="not below its modulus"):
        rp.ring_decrypt(bad, s, meta)
    with pytest.raises(ValueError, match="does not belong"):
        rp.ring_decrypt(arr, s, dict(meta, ring=3))
    with pytest.raises(ValueError, match="does not belong"):
        rp.ring_decrypt(np.zeros((2, 2, 16384), np.uint32), np.zeros(16384, np.int32), dict(meta, ring=16384))

    class Ctx:
        engine = _Engine(13)

        def ring_secret(self, ring):
            return np.zeros(ring, np.int32)

    pack = dict(members=2, G=2, period=256, slots=4096, present=[True, True], layouts=[None, None], value_dtypes=[None, None], **{k: meta[k] for k in ("ring", "moduli", "scale")})
    with pytest.raises(ValueError, match="do not fit"):
        rp.unpack_results(Ctx(), arr, pack)                              # 2 G period = 1024 > 512
    out = rp.unpack_results(Ctx(), arr, dict(pack, period=64))
    assert len(out) == 2 and out[0].shape == (4096,)


def test_meta_survives_json_and_the_bound_reads_it():
    meta = dict(members=1, G=1, period=16, slots=4096, present=[True], layouts=[None], value_dtypes=[None], ring=512, moduli=list(Q), scale=SCALE,
                special=[1073479681, 1073479679])
    again = json.loads(json.dumps(meta))
    assert again == meta
    coef = rp.ring_switch_bound(again, coefficient=True)
    p = 1073479681.0 * 1073479679.0
    assert coef == pytest.approx(2 * max(Q) * 8192 * 6 * np.sqrt(10.5) / p + 513 / 2)
    assert rp.ring_switch_bound(again) == pytest.approx(512 * coef / SCALE)
    one = dict(again, special=[1073479681], ring=4096, scale=966367641.6)   # the engine's delta_0 target, 0.9 * 2^30
    assert rp.ring_switch_bound(one) > 0.5 / 256                         # one special prime: vacuous for 8-bit values, as §3.29 says
