"""Residue rows at the edges of [0, q): the inputs of the bit-exact edge tests (tests/test_gpu_edge_residues.py,
tests/test_gpu_keyswitch_shapes.py).  Uniform residues meet a boundary such as a + b == q, x == 2q or a quotient
estimate off by two about once in 2^30 words, and sums of uniform products sit near half their bound; these rows
sit on the boundaries and at the bounds.  Pure numpy; `ntt_top` and `conv_top` transform through the CPU oracle
(an oracle.ckks_cpu.OracleParams).  Every residue is below its row's modulus."""
import numpy as np

IMPULSES = ("impulse_first", "impulse_mid", "impulse_last")
BASIC = ("zero", "top", "alt", "alt_c") + IMPULSES + ("corners",)


def _col(moduli):
    q = np.asarray(moduli, np.uint64).reshape(-1)
    if q.size == 0 or (q < 5).any() or (q >= 1 << 32).any() or not (q & 1).all():
        raise ValueError("moduli: odd primes below 2^32")
    return q[:, None]


def zero(moduli, n):
    return np.zeros((len(_col(moduli)), n), np.uint32)


def top(moduli, n):
    """q - 1 in every word"""
    return np.broadcast_to(_col(moduli) - 1, (len(_col(moduli)), n)).astype(np.uint32)


def alt(moduli, n, complement=False):
    """0, q - 1, 0, q - 1, ... by coefficient index; complement: q - 1 first"""
    out = zero(moduli, n)
    t = top(moduli, n)
    s = slice(0, None, 2) if complement else slice(1, None, 2)
    out[:, s] = t[:, s]
    return out


def impulse(moduli, n, index):
    """a single q - 1 at `index`, zeros elsewhere"""
    out = zero(moduli, n)
    out[:, index] = (_col(moduli) - 1)[:, 0]
    return out


def corner_values(moduli):
    """[rows][7]: 0, 1, 2, q - 2, q - 1, (q - 1) / 2, (q + 1) / 2 -- the words at which a >= written as > , a missed
    conditional subtraction or a doubled value crossing q first shows"""
    q = _col(moduli)
    return np.concatenate([0 * q, 0 * q + 1, 0 * q + 2, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2], axis=1)


def corners(moduli, n, seed):
    """each word drawn uniformly from corner_values of its row"""
    v = corner_values(moduli)
    pick = np.random.default_rng(seed).integers(0, v.shape[1], (v.shape[0], n))
    return np.take_along_axis(v, pick, axis=1).astype(np.uint32)


def uniform(moduli, n, seed):
    """uniform residues (what the older parity tests draw): the baseline beside the edge rows"""
    q = _col(moduli)
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, int(m), n, dtype=np.uint64) for m in q[:, 0]]).astype(np.uint32)


def basic(moduli, n, seed):
    """name -> [len(moduli)][n] rows of every pattern that needs no transform"""
    out = {"zero": zero(moduli, n), "top": top(moduli, n), "alt": alt(moduli, n), "alt_c": alt(moduli, n, True)}
    for name, k in zip(IMPULSES, (0, n // 2, n - 1)):
        out[name] = impulse(moduli, n, k)
    out["corners"] = corners(moduli, n, seed)
    return out


def ntt_top(O, limbs):
    """(fwd_in, inv_in): the rows whose forward transform is all q - 1 (the oracle's inverse transform of `top`), and
    the rows whose inverse transform is all q - 1 (its forward transform of `top`), on the oracle's primes `limbs`"""
    limbs = list(limbs)
    t = top(O.moduli[limbs], O.n)
    return O.intt(t, limbs), O.ntt(t, limbs)


def conv_weights(q):
    """(qhat_i mod q_i, qhat_i^-1 mod q_i) of the base-conversion source group q, qhat_i = prod_{j != i} q_j"""
    q = [int(x) for x in q]
    hat = []
    for i, qi in enumerate(q):
        v = 1
        for j, qj in enumerate(q):
            if j != i:
                v = v * qj % qi
        hat.append(v)
    return hat, [pow(h, -1, qi) for h, qi in zip(hat, q)]


def conv_top(O, limbs):
    """NTT-form rows on the source group `limbs` of one base conversion whose coefficient form is the constant
    c_i = -qhat_i mod q_i in every word: every conversion source y_i = c_i qhat_i^-1 is then q_i - 1, the largest
    addends and the largest overflow estimate the conversion can meet"""
    limbs = list(limbs)
    q = O.moduli[limbs]
    hat, _ = conv_weights(q)
    c = np.array([(int(qi) - h) % int(qi) for h, qi in zip(hat, q)], np.uint32)
    return O.ntt(np.broadcast_to(c[:, None], (len(limbs), O.n)).astype(np.uint32), limbs)


def conv_top_digits(O, nl, alpha):
    """conv_top of every key-switching digit of a polynomial of nl limbs (digits of alpha limbs, the last one
    partial): the d operand that saturates every ModUp conversion at once"""
    return np.concatenate([conv_top(O, range(lo, min(lo + alpha, nl))) for lo in range(0, nl, alpha)])


# ----------------------------------------------------------------------------- plaintexts with known residues
# A slot vector z = embed(m) / scale encodes, at `scale`, to the small integer polynomial m exactly: the inverse
# embedding returns m / scale to a relative 1e-13 or so, the product with the scale is m to far better than 1/2,
# and the encoder's rounding lands on m.  The plaintext residues on every Q and P row are then NTT(m mod q) -- known
# without trusting either float encoder (tests/test_oracle_hoisted.py asserts it of the oracle's, the GPU parity
# tests of the engine's).  Each builder returns (z, m): the slots to hand to encode, and the int64 polynomial.
def pt_scale(scales, moduli, level, nl=lambda l: l + 2):
    """the engine's plaintext scale of `level` (csrc/params.cpp ptscale[l]), the same expression in the same order:
    scales = E.scales() / O.deltas, moduli = E.moduli() / O.moduli"""
    qd = 1.0
    for t in range(nl(level - 1), nl(level)):
        qd *= float(moduli[t])
    return float(scales[level - 1]) * qd / float(scales[level])


def pt_from_poly(O, m, scale):
    """(z, m) for any integer polynomial m with |m_k| well below 2^40; z is never constant across the slots (the
    engines take a constant plaintext as a scalar by exact equality): a constant one has slot 1 nudged by a
    relative 1e-12, which moves no coefficient by more than 1e-12 |m_0|"""
    m = np.asarray(m, np.int64).reshape(-1)
    if m.shape != (O.n,) or np.abs(m).max() >= 1 << 40:
        raise ValueError("pt_from_poly: N small integer coefficients")
    z = O.embed(m.astype(np.float64)) / float(scale)
    if np.all(z == z[0]):
        z = z.copy()
        z[1] = z[1] * (1.0 + 1e-12)
    assert not np.all(z == z[0])
    return z, m


def pt_top(O, scale):
    """m = -1: every residue of the NTT form is q - 1, on every row, special primes included"""
    m = np.zeros(O.n, np.int64)
    m[0] = -1
    return pt_from_poly(O, m, scale)


def pt_impulse(O, scale, k=None):
    """m = -X^k (k = N / 2 + 1 unless given): the NTT form is minus a power of each row's 2N-th root per word,
    residues over the whole of [0, q)"""
    m = np.zeros(O.n, np.int64)
    m[O.n // 2 + 1 if k is None else k] = -1
    return pt_from_poly(O, m, scale)


def pt_small(O, scale, seed):
    """random coefficients in +-2^20: a mask of ordinary size, every residue different"""
    m = np.random.default_rng(seed).integers(-(1 << 20), (1 << 20) + 1, O.n)
    return pt_from_poly(O, m, scale)


def poly_ntt(O, m, limbs):
    """NTT form of the integer polynomial m on the oracle's primes `limbs`: [len(limbs)][N]"""
    limbs = list(limbs)
    q = O.moduli[limbs].astype(np.int64)[:, None]
    return O.ntt((np.asarray(m, np.int64)[None, :] % q).astype(np.uint32), limbs)
