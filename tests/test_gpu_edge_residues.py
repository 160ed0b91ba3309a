"""Bit-exact parity with the CPU oracle at EDGE residues (tests/helpers/edge_patterns.py): the older parity tests
draw residues uniformly, so a + b == q, x == 2q in a lazy reduction, v == 0 in the negation, or a Barrett / Shoup
quotient estimate at its worst meet a word about once in 2^30, and sums of uniform products sit near half their
bound.  Here every NTT path (log N 13 .. 16, the small launch and the 512-thread column pass, rows across the
Q | P boundary), the element-wise kernels, rescale, level alignment, tensor, the relinearised product, the rotation
and the fused LUT sums at their full size (16 x 16 terms, kLutChunk univariate terms) run on rows of 0, q - 1 and the
other corner values.  Every comparison is np.array_equal; no tolerance anywhere."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import ROOT, gpu_engine

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import edge_patterns as ep  # noqa: E402
from test_gpu_lut import llround, ntt_const, raw_scale  # noqa: E402  the LUT tests' oracle model

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def kernels_h_const(name):
    m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", (ROOT / "aes-implementation-fhe_amd" / "csrc" / "kernels.h").read_text())
    assert m, name
    return int(m.group(1))


# ---------------------------------------------------------------------------------------------------- NTT
@pytest.fixture(scope="module", params=[13, 14, 15, 16], ids=lambda n: f"logn{n}")
def ntt_pair(request):
    """max_level 17, dnum 3: 20 Q primes (the encryption limb included) + 8 special primes = 28 rows; debug_ntt
    needs no key, so nothing is generated"""
    from mi355x_ckks import Engine
    from oracle.ckks_cpu import OracleParams
    log_n = request.param
    E = gpu_engine(log_n=16, max_level=17, seed=SEED) if log_n == 16 else \
        Engine(log_n=log_n, max_level=17, dnum=3, seed=SEED, allow_insecure=True, enc_nonce=SEED)
    O = OracleParams(log_n=log_n, max_level=17, dnum=3, seed=SEED)
    assert np.array_equal(E.moduli(), O.moduli) and O.n_q + O.n_p == 28
    return E, O


def ntt_ranges(O):
    """(first prime, rows): 3 rows (the small launch, 256-thread column blocks) and >= 16 rows (the 512-thread
    column pass), each once inside Q and once across the Q | P boundary, and all 28 rows"""
    return [(0, 3), (O.n_q - 1, 3), (0, 16), (O.n_q - 9, 17), (0, O.n_q + O.n_p)]


def test_ntt_edge_rows_bitexact(ntt_pair):
    E, O = ntt_pair
    for first, rows in ntt_ranges(O):
        limbs = list(range(first, first + rows))
        q = O.moduli[limbs]
        pats = ep.basic(q, O.n, 100 + first + rows)
        pats["ntt_top_fwd"], pats["ntt_top_inv"] = ep.ntt_top(O, limbs)
        for name, x in pats.items():
            assert np.array_equal(E.debug_ntt(x, first), O.ntt(x, limbs)), (name, first, rows, "forward")
            assert np.array_equal(E.debug_ntt(x, first, inverse=True), O.intt(x, limbs)), (name, first, rows, "inverse")
        # closed form, no oracle in the loop: these rows transform to q - 1 in every word
        t = ep.top(q, O.n)
        assert np.array_equal(E.debug_ntt(pats["ntt_top_fwd"], first), t), (first, rows)
        assert np.array_equal(E.debug_ntt(pats["ntt_top_inv"], first, inverse=True), t), (first, rows)


# --------------------------------------------------------------- element-wise, rescale, tensor, automorphism
@pytest.fixture(scope="module")
def pair():
    from oracle.ckks_cpu import OracleParams
    return gpu_engine(log_n=13, max_level=6, seed=SEED), OracleParams(log_n=13, max_level=6, dnum=3, seed=SEED)


def edge_cts(O, level, seed):
    """name -> [2][level + 2][N] ciphertext rows: both polynomials of a pattern (corners: two draws)"""
    q = O.moduli[: level + 2]
    out = {k: np.stack([v, v]) for k, v in ep.basic(q, O.n, seed).items() if k in ("top", "alt", "zero")}
    out["corners"] = np.stack([ep.corners(q, O.n, seed), ep.corners(q, O.n, seed + 1)])
    return out


OPERAND_PAIRS = [("top", "top"), ("corners", "corners"), ("corners", "top"), ("alt", "corners"), ("zero", "top"), ("alt", "alt")]


def test_add_sub_neg_edge_bitexact(pair):
    E, O = pair
    level = 5
    q = O.limbs_mod(level + 2)
    A, B = edge_cts(O, level, 11), edge_cts(O, level, 13)
    for na, nb in OPERAND_PAIRS:
        a, b = A[na], B[nb]
        ca, cb = E.import_ct(a, level), E.import_ct(b, level)
        a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
        assert np.array_equal(E.export(E.add(ca, cb)), ((a64 + b64) % q).astype(np.uint32)), (na, nb)
        assert np.array_equal(E.export(E.subtract(ca, cb)), ((a64 + q - b64) % q).astype(np.uint32)), (na, nb)
        assert np.array_equal(E.export(E.subtract(cb, ca)), ((b64 + q - a64) % q).astype(np.uint32)), (na, nb)
    for name in ("corners", "top", "alt", "zero"):
        a = A[name]
        a64 = a.astype(np.uint64)
        ca = E.import_ct(a, level)
        # a + (q - a): every sum is exactly q (0 where a is 0) -> all zeros
        comp = ((q - a64) % q).astype(np.uint32)
        assert not E.export(E.add(ca, E.import_ct(comp, level))).any(), name
        # a - a: the same ciphertext (the engine's zero shortcut) and an equal copy (the subtraction kernel at a == b)
        assert not E.export(E.subtract(ca, ca)).any(), name
        assert not E.export(E.subtract(ca, E.import_ct(a.copy(), level))).any(), name
        # 0 - a: the negation kernel, v == 0 included (must stay 0, not q)
        z = E.subtract(ca, ca)
        assert np.array_equal(E.export(E.subtract(z, ca)), comp), name
        # a + a: doubles (q - 1) / 2 and (q + 1) / 2 to q - 1 and q + 1
        assert np.array_equal(E.export(E.add(ca, E.import_ct(a.copy(), level))), (2 * a64 % q).astype(np.uint32)), name


def test_rescale_tensor_edge_bitexact(pair):
    E, O = pair
    level = 5
    A, B = edge_cts(O, level, 21), edge_cts(O, level, 23)
    for name, a in A.items():
        assert np.array_equal(E.export(E.rescale(E.import_ct(a, level))), O.rescale(level, a)), name
    for na, nb in OPERAND_PAIRS:
        a, b = A[na], B[nb]
        got = E.export(E.multiply(E.import_ct(a, level), E.import_ct(b, level)))
        assert np.array_equal(got, O.tensor(level, a, b)), (na, nb)


def test_relin_rescale_edge_bitexact(pair):
    """the relinearised, rescaled product under the engine's own key, as test_rescale_tensor_automorph_bitexact"""
    E, O = pair
    key = O.gen_ksk(0)
    for lv in (1, 3, O.L - 1):
        X, Y = edge_cts(O, lv, 31 + lv), edge_cts(O, lv, 37 + lv)
        qq = O.limbs_mod(lv + 2)
        for na, nb in OPERAND_PAIRS:
            x, y = X[na], Y[nb]
            t2 = O.tensor(lv, x, y)
            ks = O.keyswitch(lv, t2[2], key)
            relin = ((t2[:2].astype(np.uint64) + ks) % qq).astype(np.uint32)
            got = E.export(E.multiply(E.import_ct(x, lv), E.import_ct(y, lv), "rlk"))
            assert np.array_equal(got, O.rescale(lv, relin)), (lv, na, nb)


def test_rotation_edge_bitexact(pair):
    E, O = pair
    level = 5
    q = O.limbs_mod(level + 2)
    steps = E.slot_count // 8
    g = E.galois_rotate(steps)
    key = O.gen_ksk(g)
    for name, a in edge_cts(O, level, 41).items():
        x = O.automorph(level, g, a)
        ks = O.keyswitch(level, x[1], key)
        ks[0] = ((ks[0].astype(np.uint64) + x[0]) % q).astype(np.uint32)
        assert np.array_equal(E.export(E.rotate(E.import_ct(a, level), None, steps)), ks), name


def test_level_down_edge_bitexact(pair):
    E, O = pair
    a_lv, b_lv = O.L, 2
    c = int(round(O.deltas[b_lv] * float(O.moduli[b_lv + 2]) / O.deltas[a_lv]))
    consts = O.const_residues(c, b_lv + 3)
    for name, a in edge_cts(O, a_lv, 51).items():
        x = O.mul_limb_consts(consts, np.ascontiguousarray(a[:, : b_lv + 3]))
        assert np.array_equal(E.export(E.level_down(E.import_ct(a, a_lv), b_lv)), O.rescale(b_lv + 1, x)), name


# ------------------------------------------------------------------------------- fused LUT sums at full size
def lut_operand(O, level, kind, seed):
    q = O.moduli[: level + 2]
    if kind == "top":
        return np.stack([ep.top(q, O.n)] * 2)
    return np.stack([ep.corners(q, O.n, seed), ep.corners(q, O.n, seed + 1000)])


@pytest.mark.parametrize("kind", ["corners", "top"])
def test_bivariate_lut_16x16_edge_bitexact(pair, kind):
    """kLutMax x kLutMax terms, every coefficient non-zero (AES's tables are 16 x 16; test_bivariate_lut_bitexact
    runs 3 x 3): 16 terms per A element and 16 A elements through the kernel's lazy sums.  The oracle model is
    test_bivariate_lut_bitexact's."""
    E, O = pair
    n = kernels_h_const("kLutMax")
    assert n == 16
    rng = np.random.default_rng(61)
    top = O.L
    la = [top - (p % 2) for p in range(n)]
    lb = [top - (1 if qq % 3 == 0 else 0) for qq in range(n)]
    A = [lut_operand(O, lv, kind, 200 + p) for p, lv in enumerate(la)]
    B = [lut_operand(O, lv, kind, 300 + p) for p, lv in enumerate(lb)]
    C = rng.uniform(0.25, 1.0, (n, n)) * np.exp(2j * np.pi * rng.random((n, n)))
    C[0, 0] = 0.75  # a real coefficient
    assert np.all(C != 0)
    lut = E.lut_create(C)
    out = E.lut_eval(lut, [E.import_ct(a, lv) for a, lv in zip(A, la)], [E.import_ct(b, lv) for b, lv in zip(B, lb)])
    l = min(la + lb)
    nl = l + 2
    assert out.level == l - 2
    q = O.limbs_mod(nl).astype(np.uint64)
    s_out = raw_scale(O, l, 2)
    raw = np.zeros((3, nl, O.n), np.uint64)
    for p in range(n):
        for qq in range(n):
            f = s_out / (float(O.deltas[la[p]]) * float(O.deltas[lb[qq]]))
            k = ntt_const(O, llround(C[p, qq].real * f), llround(C[p, qq].imag * f), nl)
            t = O.tensor(l, A[p][:, :nl], B[qq][:, :nl]).astype(np.uint64)
            raw = (raw + t * k % q) % q
    r1 = O.rescale(l, raw.astype(np.uint32)).astype(np.uint64)
    ks = O.keyswitch(l - 1, r1[2].astype(np.uint32), O.gen_ksk(0)).astype(np.uint64)
    relin = ((r1[:2] + ks) % O.limbs_mod(nl - 1).astype(np.uint64)).astype(np.uint32)
    assert np.array_equal(E.export(out), O.rescale(l - 1, relin))
    E.lut_free(lut)


@pytest.mark.parametrize("extra", [0, 1], ids=["chunk", "chunk_plus_1"])
@pytest.mark.parametrize("kind", ["corners", "top"])
def test_univariate_lut_full_chunk_edge_bitexact(pair, kind, extra):
    """kLutChunk terms: the most one k_lut_univariate launch sums, every coefficient non-zero.  lut_create sets no
    limit on a univariate table: lut_eval passes a longer one through in chunks of that size, each launch adding
    to the last one's output -- kLutChunk + 1 terms cross that boundary.  Model: test_univariate_lut_bitexact's."""
    E, O = pair
    n = kernels_h_const("kLutChunk") + extra
    rng = np.random.default_rng(62)
    top = O.L
    lv = [top - (k % 2) for k in range(n)]
    X = [lut_operand(O, v, kind, 400 + k) for k, v in enumerate(lv)]
    C = rng.uniform(0.25, 1.0, n) * np.exp(2j * np.pi * rng.random(n))
    c0 = 0.3 - 0.8j
    lut = E.lut_create(C, c0)
    out = E.lut_eval(lut, [E.import_ct(x, v) for x, v in zip(X, lv)])
    l = min(lv)
    nl = l + 2
    assert out.level == l - 1
    q = O.limbs_mod(nl).astype(np.uint64)
    s_out = raw_scale(O, l, 1)
    raw = np.zeros((2, nl, O.n), np.uint64)
    for x, v, c in zip(X, lv, C):
        f = s_out / float(O.deltas[v])
        raw = (raw + x[:, :nl].astype(np.uint64) * ntt_const(O, llround(c.real * f), llround(c.imag * f), nl) % q) % q
    k0 = ntt_const(O, llround(c0.real * float(O.deltas[l - 1])), llround(c0.imag * float(O.deltas[l - 1])), nl)
    f0 = np.array([int(O.moduli[l + 1]) % int(O.moduli[t]) for t in range(nl)], np.uint64)
    raw[0] = (raw[0] + k0 * f0[:, None] % q) % q
    assert np.array_equal(E.export(out), O.rescale(l, raw.astype(np.uint32)))
    E.lut_free(lut)
