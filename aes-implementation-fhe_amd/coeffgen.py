"""Coefficient generator for the Zeta16 LUT polynomials.

Produces the same JSON files the reference ships in REF/gen/coeff/ (format read by
REF/lut.py:10-62) from truth tables, by inverse DFT over the 16th / 256th roots of
unity ζ = e^{-2πi/n}:

* 8->4 LUTs (SubBytes / InvSubBytes / split), REF/gen/generate_sobx_coeffs.py:65-120:
  a_k = (1/256) Σ_j ζ16^{f(j)} ζ256^{-jk}, so Σ_k a_k (ζ256^j)^k = ζ16^{f(j)}.
* GF(2^8) constant multipliers on (hi, lo) nibbles, REF/gen/generate_gf_mult_2var_coeff.py:15-113:
  c[p,q] = (1/256) Σ_{h,l} ζ16^{nib(k·(16h+l))} ζ16^{-(ph+ql)}.
* 4-bit XOR, REF/gen/generate_xor4_coeffs.py:10-54 -- keeps the reference's n^2 factor
  (REF/gen/generate_xor4_coeffs.py:17): Σ c[p,q] x^p y^q = 256·ζ16^{a⊕b}
  (the pipeline's renorm re-anchors the magnitude).
* Zeta16 snap polynomial (REF/gen/make_zeta16_snap_coeffs.py:11-56): ridge
  least-squares fit of z -> nearest ζ16 codeword on the unit circle.

Run ``python coeffgen.py [outdir]``; the engine's modules load ./coeff/ by default.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

COEFF_DIR = Path(__file__).resolve().parent / "coeff"


def _gf_mul(a: int, b: int) -> int:
    out = 0
    while b:
        if b & 1:
            out ^= a
        a = ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF
        b >>= 1
    return out


def _sboxes():
    inv = [0] * 256
    for x in range(1, 256):
        inv[x] = next(y for y in range(1, 256) if _gf_mul(x, y) == 1)
    rotl = lambda b, k: ((b << k) | (b >> (8 - k))) & 0xFF
    s = [inv[x] ^ rotl(inv[x], 1) ^ rotl(inv[x], 2) ^ rotl(inv[x], 3) ^ rotl(inv[x], 4) ^ 0x63 for x in range(256)]
    si = [0] * 256
    for x, y in enumerate(s):
        si[y] = x
    return s, si


def _zeta(n: int) -> complex:
    return np.exp(-2j * np.pi / n)


def lut_8to4(table) -> np.ndarray:
    """256-point inverse DFT of ζ16^{table[j]} (1-D LUT over ζ256 inputs)."""
    samples = _zeta(16) ** np.asarray(table, dtype=np.int64)
    return np.fft.ifft(samples)


def lut_bivariate(f, scale: float = 1.0) -> np.ndarray:
    """c[p,q] with Σ c[p,q] ζ16^{ph+ql} = scale·ζ16^{f(h,l)}."""
    F = np.array([[_zeta(16) ** f(h, l) for l in range(16)] for h in range(16)])
    return np.fft.ifft2(F) * scale


def xor_value_table(signed: bool = False) -> np.ndarray:
    """E[p, b] = (1/16) Σ_k (k ⊕ b) ζ16^{-pk}: the INTEGER value of a ⊕ b for a Zeta16 nibble a = ζ16^k and a
    public nibble b is Σ_p E[p, b] a^p (xor_value_lut.py).  Closed form, with w = ζ16^{-p}:
    k ⊕ b = k + b - 2 Σ_j 2^j b_j k_j over the bits j; Σ_k k w^k is 120 at p = 0 and 16 / (w - 1) elsewhere;
    Σ_{k: k_j = 1} w^k is 8 at p = 0, 2^(4-j) / (w - 1) where p is an odd multiple of 2^(3-j), and 0 elsewhere.
    Every p > 0 is an odd multiple of exactly one 2^(3-j), j(p) = 3 - v2(p), so
        E[0, b] = 7.5,        E[p, b] = (-1)^(bit j(p) of b) / (ζ16^{-p} - 1)   (p > 0):
    E[8] = -+1/2 is real, E[16 - p] = conj(E[p]), no entry is zero, max |E[p]| = 1 / (2 sin(π/16)) = 2.563 at p = 1.
    signed=True: the table Es of the SIGNED value sval(x) = x - 16 [x >= 8] of a ⊕ b (a two's-complement top nibble,
    DESIGN.md §3.21).  Only bit 3 changes weight (8 -> -8) and j(p) = 3 exactly for the odd p, so Es is E with the odd
    rows negated and Es[0] = 7.5 - 8 = -0.5; Es[8] stays real and Es[16 - p] = conj(Es[p])."""
    E = np.full((16, 16), 7.5, np.complex128)
    b = np.arange(16)
    for p in range(1, 16):
        j = 3 - ((p & -p).bit_length() - 1)
        E[p] = (1.0 - 2.0 * ((b >> j) & 1)) / (_zeta(16) ** -p - 1.0)
    E[8] = E[8].real  # ζ16^{-8} = -1 up to an ulp of imaginary part
    if signed:
        E[1::2] *= -1.0
        E[0] -= 8.0
    return E


BYTE_LUT_Q = tuple(range(-7, 9))  # the lo-side exponents q of byte_value_table, in the order of its q index (q + 7)


def _byte_table(f) -> np.ndarray:
    f = np.asarray(f, np.float64)
    if f.shape != (256,) or not np.all(np.isfinite(f)):
        raise ValueError(f"a byte table is 256 finite reals, got shape {f.shape}")
    return f


def byte_value_table(f):
    """(K, C_00) for a 256-entry real table f (xor_value_lut.ByteValueLUT).  A byte x = 16 x_hi + x_lo
    with Zeta16 codewords a = ζ16^x_hi, c = ζ16^x_lo and a public byte b = 16 b_hi + b_lo:
        f(x ⊕ b) = Σ_{p,q<16} C_pq[b] a^p c^q,   C_pq[b] = (1/256) Σ_{k,l<16} f(16 (k ⊕ b_hi) + (l ⊕ b_lo)) ζ16^{-pk-ql}.
    f is real, so C_(-p,-q) = conj(C_pq): C_00 = mean(f) whatever b is, C_08, C_80 and C_88 are real, and
        f(x ⊕ b) = C_00 + T + conj(T),   T = Σ_{q=-7..8} y_q U_q,   U_q = Σ_{p=0..8} K_pq[b] a^p,
    y_q = c^q (q >= 0, y_0 = 1), conj(c^-q) (q < 0).  K[p, q + 7, b] (9 x 16 x 256 complex) holds one of every
    conjugate pair: K_pq = C_{p, q mod 16} for p = 1..7 and every q; K_0q = C_0q and K_8q = C_8q for q = 1..7; the real
    self-conjugate C_08, C_88, C_80 enter as halves at (0, 8), (8, 8), (8, 0); every other entry is 0."""
    f = _byte_table(f)
    b = np.arange(256)
    k, l = np.indices((16, 16))
    g = f[16 * (k[None] ^ (b >> 4)[:, None, None]) + (l[None] ^ (b & 15)[:, None, None])]  # [b][k][l]
    C = np.moveaxis(np.fft.fft2(g, axes=(1, 2)) / 256.0, 0, -1)  # fft's e^(-2 pi i pk / 16) is ζ16^(pk): C[p][q][b]
    C = C[(-np.arange(16)) % 16][:, (-np.arange(16)) % 16]       # ... so index (p, q) -> (-p, -q)
    K = np.zeros((9, 16, 256), np.complex128)
    for qi, q in enumerate(BYTE_LUT_Q):
        K[1:8, qi] = C[1:8, q % 16]
        if 1 <= q <= 7:
            K[0, qi], K[8, qi] = C[0, q], C[8, q]
    K[0, 8 + 7] = 0.5 * C[0, 8].real
    K[8, 8 + 7] = 0.5 * C[8, 8].real
    K[8, 0 + 7] = 0.5 * C[8, 0].real
    return K, float(C[0, 0, 0].real)


def byte_value_eval(K, c00, b, a, c):
    """C_00 + T + conj(T) of byte_value_table's K at public bytes b and (possibly perturbed) codewords a, c"""
    b = np.asarray(b)
    T = 0.0
    for qi, q in enumerate(BYTE_LUT_Q):
        y = c ** q if q >= 0 else np.conj(c ** -q)
        T = T + y * sum(K[p, qi, b] * a ** p for p in range(9))
    return c00 + T + np.conj(T)


def byte_value_sensitivity(f, eps: float = 1e-4) -> float:
    """max |F(perturbed) - f| / eps over all bytes x (public byte 0) and the four sign combinations, F the formula of
    byte_value_table with both codewords perturbed to ζ16^k e^(+-i eps) (1 +- eps): how much the decode amplifies a
    codeword error, per unit of it (§3.20's 930 figure for the byte value, in table units)"""
    f = _byte_table(f)
    K, c00 = byte_value_table(f)
    x = np.arange(256)
    zero = np.zeros(256, np.int64)
    worst = 0.0
    for sa in (1.0, -1.0):
        for sr in (1.0, -1.0):
            d = np.exp(1j * sa * eps) * (1.0 + sr * eps)
            F = byte_value_eval(K, c00, zero, _zeta(16) ** (x >> 4) * d, _zeta(16) ** (x & 15) * d)
            worst = max(worst, float(np.abs(F - f).max()))
    return worst / eps


def _entries_1d(a, tol):
    return [[int(k), float(c.real), float(c.imag)] for k, c in enumerate(a) if abs(c) > tol]


def _entries_2d(A, tol):
    return [[int(p), int(q), float(A[p, q].real), float(A[p, q].imag)]
            for p in range(A.shape[0]) for q in range(A.shape[1]) if abs(A[p, q]) > tol]


def snap_poly(deg: int = 15, n_samples: int = 8192, ridge: float = 1e-5) -> np.ndarray:
    theta = np.linspace(0, 2 * np.pi, n_samples, endpoint=False)
    x = np.exp(1j * theta)
    k = np.round((theta % (2 * np.pi)) / (2 * np.pi / 16)).astype(np.int64) % 16
    y = np.exp(1j * 2 * np.pi * k / 16.0)
    V = x[:, None] ** np.arange(deg + 1)[None, :]
    A = V.conj().T @ V + ridge * np.eye(deg + 1)
    return np.linalg.solve(A, V.conj().T @ y)


def generate(out_dir: Path = COEFF_DIR) -> dict:
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    sbox, inv_sbox = _sboxes()
    files = {}

    def put(name, obj, indent=2):
        files[name] = obj
        (out_dir / name).write_text(json.dumps(obj, indent=indent), encoding="utf-8")

    one_d = {
        "split_mod256_to_16_hi.json": [x >> 4 for x in range(256)],
        "split_mod256_to_16_lo.json": [x & 15 for x in range(256)],
        "mod256_to_16_hi.json": [y >> 4 for y in sbox],
        "mod256_to_16_lo.json": [y & 15 for y in sbox],
        "inv_mod256_to_16_hi.json": [y >> 4 for y in inv_sbox],
        "inv_mod256_to_16_lo.json": [y & 15 for y in inv_sbox],
    }
    for name, table in one_d.items():
        put(name, {"entries": _entries_1d(lut_8to4(table), 1e-12)})

    for mult in (1, 2, 3, 9, 11, 13, 14):
        for which, nib in (("hi", lambda y: y >> 4), ("lo", lambda y: y & 15)):
            C = lut_bivariate(lambda h, l: nib(_gf_mul((h << 4) | l, mult)))
            put(f"gf_mult{mult}_{which}_coeffs.json",
                {"entries": _entries_2d(C, 1e-12), "multiplier": mult, "which": which, "domain": "zeta16", "size": 16},
                indent=0)

    put("xor4_coeffs.json", {"entries": _entries_2d(lut_bivariate(lambda a, b: a ^ b, 256.0), 1e-8)})
    put("zeta16_snap_coeffs.json", {"type": "zeta16_snap_1d_poly", "entries": _entries_1d(snap_poly(), -1.0)})
    return files


if __name__ == "__main__":
    generate(Path(sys.argv[1]) if len(sys.argv) > 1 else COEFF_DIR)
