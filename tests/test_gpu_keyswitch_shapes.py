"""The key switch at its digit extremes, bit for bit against the CPU oracle, with keys and operands at the edges.

The hand-derived bounds of the key switch bind at shapes no other test runs: base conversions of 9 .. 16 sources
(k_base_convert's conv_body<H, V>: H = 15 sums fifteen 60-bit products with no fold, H = 16 is the one instantiation
that folds), inner products of more than 8 digits (the fold every 8 terms, the run-time digit loop of k_key_inner),
and the relinearisation whose fused ModDown-with-rescale would need 17 sources and falls back to two steps.  An
evaluation-only engine takes any reduced key (import_ksk) and the oracle's keyswitch the same array, so neither side
generates a key and BOTH operands of the inner product are chosen: q - 1 everywhere, corner values, the rows that
make every conversion source q_i - 1 (edge_patterns.conv_top), and uniform rows as the baseline.

Sets (tests/helpers/keyswitch_shapes_probe.py): A alpha 15 / 16 special primes / 1 digit, B alpha 10 / 2 digits,
C alpha 2 / 10 digits, D alpha 1 / 19 digits, E = A at N = 2^16.  Every comparison is np.array_equal."""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import edge_patterns as ep  # noqa: E402
import keyswitch_shapes_probe as ks  # noqa: E402

pytestmark = pytest.mark.gpu

PROBE = Path(ks.__file__).resolve()
ROT_STEPS = 3
HOIST_STEPS = (3, 5)  # rotate_many: two non-zero steps, so the ModUp is hoisted and shared


class Rig:
    def __init__(self, name, kind):
        self.name, self.kind = name, kind
        self.O = O = ks.oracle(name)
        self.key = ks.make_key(O, kind)
        self.g_conj = O.galois_conj
        self.g_rot = O.galois_rotate(ROT_STEPS)
        self.g_hoist = [O.galois_rotate(s) for s in HOIST_STEPS]
        # one key under every tag the calls look up: relinearisation (0), the rotations', the conjugation's
        self.E = ks.build_engine(name, O, self.key, tags=sorted({0, self.g_rot, self.g_conj, *self.g_hoist}))

    def ct(self, level, kind, seed):
        """[2][nl][N]: c0 corners, c1 -- the polynomial a rotation / conjugation key-switches -- the pattern"""
        q = self.O.moduli[: self.O.nl(level)]
        return np.stack([ep.corners(q, self.O.n, seed), ks.make_d(self.O, level, kind, seed + 1)])


@pytest.fixture(scope="module", params=[(s, k) for s in ks.SETS for k in ks.KEY_KINDS], ids=lambda p: f"{p[0]}_{p[1]}")
def rig(request):
    r = Rig(*request.param)
    yield r
    del r.E


def test_raw_core_bitexact(rig):
    """debug_keyswitch == the oracle's keyswitch at the top level, a middle level and level 0"""
    E, O = rig.E, rig.O
    for level in ks.levels(O):
        for dk in ks.D_KINDS:
            d = ks.make_d(O, level, dk)
            got = E.debug_keyswitch(level, 0, d)
            assert np.array_equal(got, O.keyswitch(level, d, rig.key)), (level, dk)
            if dk == "top" and rig.kind == "top":
                # closed form: every digit extends to -1 and every key word is -1, so both sums are the digit count nd
                # on every row of Q P -- the integer nd < P / 2, which the ModDown rounds to 0.  An accumulator that
                # overflowed at nd (q - 1)^2 would not give it
                assert not got.any(), level


def test_relin_rescale_bitexact(rig):
    """multiply(x, y, "rlk") == tensor, key switch of d2, add, rescale (test_rescale_tensor_automorph_bitexact's
    composition): eager, the inner product folds the tensor in (relin_rescale_tensor) and one ModDown divides by
    P q_l -- or, where that ModDown would need more than 16 sources (sets A and E: 16 special primes + the dropped
    limb), the two-step fallback; lazy, the materialised tensor goes through the same end on export"""
    E, O = rig.E, rig.O
    for lv in sorted({O.L, O.L // 2, 1}):
        nl = O.nl(lv)
        qq = O.limbs_mod(nl)
        for dk in ks.D_KINDS:
            x, y = rig.ct(lv, dk, 10), rig.ct(lv, dk, 20)
            if dk == "conv_top":
                x[0] = x[1]
                y[1] = 1  # NTT form of the constant 1: d2 = x1 (.) y1 is conv_top itself
            t2 = O.tensor(lv, x, y)
            kso = O.keyswitch(lv, t2[2], rig.key)
            relin = ((t2[:2].astype(np.uint64) + kso) % qq).astype(np.uint32)
            want = O.rescale(lv, relin)
            for lazy in (False, True):
                E.set_lazy(lazy)
                try:
                    got = E.export(E.multiply(E.import_ct(x, lv), E.import_ct(y, lv), "rlk"))
                finally:
                    E.set_lazy(False)
                assert np.array_equal(got, want), (lv, dk, lazy)


def galois_case(rig, lv, dk, g, call):
    E, O = rig.E, rig.O
    q = O.limbs_mod(O.nl(lv))
    a = rig.ct(lv, dk, 30)
    x = O.automorph(lv, g, a)
    want = O.keyswitch(lv, x[1], rig.key)
    want[0] = ((want[0].astype(np.uint64) + x[0]) % q).astype(np.uint32)
    assert np.array_equal(E.export(call(E.import_ct(a, lv))), want), (lv, dk)


def test_rotation_bitexact(rig):
    """rotate: a permuted copy of the ciphertext, then the plain key switch (the inner product itself reads straight)"""
    for lv in ks.levels(rig.O):
        for dk in ks.D_KINDS:
            galois_case(rig, lv, dk, rig.g_rot, lambda c: rig.E.rotate(c, None, ROT_STEPS))


def test_hoisted_rotation_bitexact(rig):
    """rotate_many: ONE ModUp of c1, then per step the inner product read THROUGH the automorphism (the gathered read
    of k_key_inner, g != 0; above 8 digits its run-time digit loop with the folds) and a ModDown adding the permuted
    c0.  Each output equals automorphism + key switch + add, as rotate's"""
    E, O = rig.E, rig.O
    for lv in ks.levels(O):
        q = O.limbs_mod(O.nl(lv))
        for dk in ks.D_KINDS:
            a = rig.ct(lv, dk, 40)
            outs = E.rotate_many(E.import_ct(a, lv), list(HOIST_STEPS))
            assert len(outs) == len(HOIST_STEPS)
            for g, out in zip(rig.g_hoist, outs):
                x = O.automorph(lv, g, a)
                want = O.keyswitch(lv, x[1], rig.key)
                want[0] = ((want[0].astype(np.uint64) + x[0]) % q).astype(np.uint32)
                assert np.array_equal(E.export(out), want), (lv, dk, g)


def test_conjugation_bitexact(rig):
    """the reversed own-digit read (rev_d) of the inner product, the reversed addend of the ModDown"""
    for lv in ks.levels(rig.O):
        for dk in ks.D_KINDS:
            galois_case(rig, lv, dk, rig.g_conj, lambda c: rig.E.conjugate(c))


# ------------------------------------------------------------------------------------- the separate launches
def test_fused_core_off_bitexact():
    """the raw core of sets A, C and D with the fused key-switch core off (AESFHE_FUSED_KI=0: k_key_inner, whose
    digit loop is a run-time loop above 8 digits) and with its 8-residue form off (AESFHE_KI8=0: k_ntt2_ki): the same
    bytes as the default run, and as the oracle.  Fresh processes -- the switches are read once -- side by side"""
    base = {k: v for k, v in os.environ.items() if k not in ("AESFHE_FUSED_KI", "AESFHE_KI8")}
    envs = {"default": base, "fused_ki_off": dict(base, AESFHE_FUSED_KI="0"), "ki8_off": dict(base, AESFHE_KI8="0")}
    procs = {k: subprocess.Popen([sys.executable, str(PROBE)], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, e in envs.items()}
    runs = {}
    try:
        for k, p in procs.items():
            out, err = p.communicate(timeout=120)
            assert p.returncode == 0, (k, err[-2000:])
            runs[k] = json.loads(out.strip().splitlines()[-1])
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    want = {}
    for name in ("A", "C", "D"):
        O = ks.oracle(name)
        for kind in ks.KEY_KINDS:
            key = ks.make_key(O, kind)
            for level in ks.levels(O):
                for dk in ks.D_KINDS:
                    r = O.keyswitch(level, ks.make_d(O, level, dk), key)
                    want[f"{name}/{kind}/{level}/{dk}"] = hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest()[:24]
    assert runs["default"] == want
    for k in ("fused_ki_off", "ki8_off"):
        bad = [c for c in want if runs[k].get(c) != runs["default"][c]]
        assert runs[k].keys() == want.keys() and not bad, (k, bad)


# ------------------------------------------------------------------------------------------------ refusals
def refusal_engine(log_n, max_level, dnum):
    from mi355x_ckks import Engine
    from oracle.ckks_cpu import OracleParams
    O = OracleParams(log_n=log_n, max_level=max_level, dnum=dnum, seed=ks.SEED)
    E = Engine.evaluation_only(prng_key=bytes(range(32)), log_n=log_n, max_level=max_level, dnum=dnum, allow_insecure=True,
                               enc_nonce=1, lazy=False, defer_calls=False)
    E.set_low_p(False)
    assert np.array_equal(E.moduli(), O.moduli)
    E.import_pk(np.zeros((2, E.n_q, E.n), np.uint32))
    return E, O


def test_refuses_17_special_primes():
    """max_level 14, one digit: alpha = 16, 17 special primes -- a ModDown of 17 sources.  Every entry point refuses
    on the host (modup's check, before any digit-shaped launch) and the engine stays usable: with the per-level
    special basis on, level 5 switches over 8 special primes, bit for bit the oracle's reduced-basis key switch.
    (On the throw debug_keyswitch and the eager product do not hand their temporary rows and the tensor back to the
    engine's pool -- a leak of that memory until the engine goes, no corruption; the hoisted form's scope does.)"""
    E, O = refusal_engine(13, 14, 1)
    assert (O.alpha, O.n_p) == (16, 17)
    key = ks.make_key(O, "top")
    for g in sorted({0, O.galois_conj, O.galois_rotate(ROT_STEPS), *(O.galois_rotate(s) for s in HOIST_STEPS)}):
        E.import_ksk(g, -1, key)
    top = O.L
    d = ks.make_d(O, top, "corners")
    a = np.stack([d, d])
    with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
        E.debug_keyswitch(top, 0, d)
    with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
        E.multiply(E.import_ct(a, top), E.import_ct(a, top), "rlk")
    with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
        E.rotate(E.import_ct(a, top), None, ROT_STEPS)
    with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
        E.conjugate(E.import_ct(a, top))
    with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
        E.rotate_many(E.import_ct(a, top), list(HOIST_STEPS))  # the hoisted ModUp: the same check
    # a legal key switch on the same engine
    E.set_low_p(True)
    lv = 5
    nl = O.nl(lv)
    assert E.ks_special_primes(lv) == nl + 1
    qk = np.concatenate([O.moduli[:nl], O.moduli[O.n_q: O.n_q + nl + 1]])
    low_key = np.stack([ep.corners(qk, O.n, 5), ep.uniform(qk, O.n, 6)])
    E.import_ksk(0, lv, low_key)
    for dk in ("corners", "top", "uniform"):
        d = ks.make_d(O, lv, dk)
        assert np.array_equal(E.debug_keyswitch(lv, 0, d), O.keyswitch_low(lv, [d], [low_key])), dk


def test_refuses_25_digits():
    """max_level 23 with 25 digits of one limb: the top level's 25 conversion groups exceed the 24 one ModUp launch
    carries and are refused on the host; one level down the 24 digits fill the launch exactly (two folds of the
    inner product) and match the oracle"""
    E, O = refusal_engine(13, 23, 25)
    assert (O.alpha, O.n_p, O.dnum) == (1, 2, 25)
    key = ks.make_key(O, "corners")
    E.import_ksk(0, -1, key)
    top = O.L
    with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
        E.debug_keyswitch(top, 0, ks.make_d(O, top, "corners"))
    for dk in ks.D_KINDS:
        d = ks.make_d(O, top - 1, dk)
        assert np.array_equal(E.debug_keyswitch(top - 1, 0, d), O.keyswitch(top - 1, d, key)), dk
