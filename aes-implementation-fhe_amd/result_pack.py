"""Result packs: several periodic results in ONE level-0 ciphertext on the download leg.

In the periodic layout a result of period P slots is a polynomial in the subring Z[X^(N / 2P)], so G such
results pack into z = sum_j X^(j k') ct_j, k' = N / (2 P G), a G P-periodic message: a sum of monomial products, exact,
with no key switch and no level (aesfhe_pack_periodic).  The server packs and exports one [2][nl(0)][N] array; the client,
who holds the secret, decrypts once and separates the members in the clear.

Slot t evaluates a polynomial at xi_t = zeta^(5^t), zeta = exp(i pi / N) (csrc/encoder.cpp; the engine's rotate by r
slots is np.roll(slots, r)), so the monomial X^e is the slot vector xi^e and

    z[t] = sum_j xi_t^(j k') m_j[t],                         m_j P-periodic.

Over the copies t + P u, u < slots / P, of one slot, 5^(P u) runs over the residues = 1 mod 4 P, each equally often, and
xi^(k') is a primitive 4 P G-th root of unity: the columns (xi_(t + P u)^(j k'))_u, j < G, are orthogonal, and

    m_j[t] = mean_u conj(xi_(t + P u))^(j k') z[t + P u].

The mean over ALL copies (not a read of the first G P slots) is the orthogonal projection onto the members' subring: it
has norm 1, so a member comes back with at most the sum of the members' own errors.

The client side (pack_slots, split_slots, unpack_results) is numpy only.

Ring-switched packs: the pack lies in Z[X^k'], so dump_results(..., ring=R) has the server key-switch it
to a secret s_R of the subring Z[X^(N / R)], R >= 2 G P, and send the coefficients at the multiples of N / R alone -- a
(2, 2, R) array, a ciphertext of the ring of degree R whose R / 2 slots are the big ring's first R / 2 (ring_decrypt,
numpy only: exact phase, CRT, the small ring's slots, tiled).
"""
from __future__ import annotations

import numpy as np

from state_encoder import _layout_tag, load_ct

MAX_MEMBERS = 32  # csrc/kernels.h kPackMembers


def group_size(count: int) -> int:
    """G: the smallest power of two >= count"""
    if not 1 <= int(count) <= MAX_MEMBERS:
        raise ValueError(f"a result pack holds 1..{MAX_MEMBERS} members, got {count}")
    g = 1
    while g < count:
        g *= 2
    return g


def _check(G: int, period: int, sc: int) -> None:
    if sc < 1 or sc & (sc - 1):
        raise ValueError(f"the slot count must be a power of two, got {sc}")
    if G < 1 or G & (G - 1) or G > MAX_MEMBERS:
        raise ValueError(f"G must be a power of two in 1..{MAX_MEMBERS}, got {G}")
    if period < 1 or period & (period - 1):
        raise ValueError(f"the period must be a power of two >= 1, got {period}")
    if G * period > sc:
        raise ValueError(f"G * period = {G * period} exceeds the {sc} slots")


def slot_exponents(sc: int) -> np.ndarray:
    """5^t mod 4 sc for t < sc: slot t evaluates at zeta^(5^t), zeta = exp(i pi / N), N = 2 sc"""
    e = np.ones(sc, np.int64)
    m = 4 * sc
    span = 1
    p5 = 5 % m  # 5^span
    while span < sc:  # doubling: e[span + i] = e[i] * 5^span
        e[span:2 * span] = e[:span] * p5 % m
        p5 = p5 * p5 % m
        span *= 2
    return e


def pack_phases(G: int, period: int, sc: int) -> np.ndarray:
    """(G, sc): row j is the slot vector of the monomial X^(j k'), k' = N / (2 period G) -- xi_t^(j k')"""
    _check(G, period, sc)
    n = 2 * sc
    kp = n // (2 * period * G)
    e = slot_exponents(sc)
    j = np.arange(G, dtype=np.int64).reshape(-1, 1)
    return np.exp(1j * np.pi * ((j * kp * e[None, :]) % (2 * n)) / n)


def _full(m, period: int, sc: int) -> np.ndarray:
    v = np.asarray(m, np.complex128)
    if v.shape == (period,):
        return np.tile(v, sc // period)
    if v.shape != (sc,):
        raise ValueError(f"a member is a vector of {period} (one period) or {sc} (all slots) entries, got shape {v.shape}")
    return v


def pack_slots(members, period: int, sc: int) -> np.ndarray:
    """The slot-level model of aesfhe_pack_periodic: z = sum_j xi^(j k') * m_j over the sc slots.  members: 1..32 vectors
    of one period (tiled here) or of all sc slots (taken slot by slot: the monomial product acts per slot, so the model
    holds for a member with noise on it too); None: an absent member"""
    members = list(members)
    G = group_size(len(members))
    ph = pack_phases(G, int(period), int(sc))
    z = np.zeros(sc, np.complex128)
    for j, m in enumerate(members):
        if m is not None:
            z += ph[j] * _full(m, period, sc)
    return z


def split_slots(z, G: int, period: int):
    """The client's split: the G members of a decrypted pack, each a full-length slot vector with its period tiled --
    m_j[t] = mean over the copies t + period u of conj(xi)^(j k') z.  Members G' >= the packed count come back ~0"""
    z = np.asarray(z, np.complex128)
    if z.ndim != 1:
        raise ValueError(f"a slot vector expected, got shape {z.shape}")
    sc = z.shape[0]
    ph = pack_phases(int(G), int(period), sc)
    m = (np.conj(ph) * z[None, :]).reshape(G, sc // period, period).mean(axis=1)
    return [np.tile(m[j], sc // period) for j in range(G)]


# ---------------------------------------------------------------- the server side
def _period_of(cts, period):
    per = None if period is None else int(period)
    tagged = []
    for c in cts:
        lay = None if c is None else getattr(c, "layout", None)
        if lay is None:
            if c is not None and per is None:
                raise ValueError("pack_results: a member without a layout tag needs an explicit period")
            continue
        if not lay.periodic:
            raise ValueError("pack_results: a member in the reference (non-periodic) slot layout cannot be packed")
        tagged.append(int(lay.period))
    if per is None:
        if not tagged:
            raise ValueError("pack_results: no member to take the period from")
        per = max(tagged)
    for p in tagged:
        if per % p:
            raise ValueError(f"pack_results: a member of period {p} does not divide the pack's period {per}")
    return per


def pack_results(ctx, cts, period=None):
    """Server side: 1..32 periodic result ciphertexts (None: an absent member) as one level-0 ciphertext with
    .pack = (G, period).  period: the members' common layout period (16 * states) by default -- the largest when they
    differ, which every other must divide; a member without a layout tag needs it given.  Runs on an evaluation-only
    context: no key, no secret.  An engine without the entry point is an error, never a CPU fallback"""
    cts = list(cts)
    group_size(len(cts))
    if all(c is None for c in cts):
        raise ValueError("pack_results: every member is absent")
    fn = getattr(ctx, "pack_periodic", None) or getattr(getattr(ctx, "engine", None), "pack_periodic", None)
    if fn is None:
        raise RuntimeError("pack_results: this engine has no aesfhe_pack_periodic entry point (rebuild the library); "
                           "there is no host fallback for packing ciphertexts")
    return fn(cts, _period_of(cts, period))


def _choose_ring(engine, G: int, period: int, ring, insecure_ok: bool) -> int:
    """the ring degree of a ring-switched pack: `ring` checked, or ("auto") the smallest power of two R < N with
    2 G period <= R that the gate accepts (any such R with insecure_ok)"""
    n, need = 2 * int(engine.slot_count), 2 * int(G) * int(period)
    mod = [int(m) for m in engine.moduli()]
    bits = float(np.log2(mod[0]) + np.log2(mod[1]) + np.log2(mod[int(engine.n_q)]))   # Q0 and ONE special prime

    def accepted(r):
        return insecure_ok or bits <= max_log_modulus(r)

    if isinstance(ring, str):
        if ring != "auto":
            raise ValueError(f"dump_results: ring is a ring degree, 'auto' or None, got {ring!r}")
        r = max(need, 2)
        while r < n and not accepted(r):
            r *= 2
        if r >= n:
            raise ValueError(f"dump_results: no ring below N = {n} holds 2 G period = {need} coefficients within the 128-bit bound "
                             f"(log2(Q0 p) = {bits:.1f})")
        return r
    r = int(ring)
    if r < 1 or r & (r - 1) or r >= n:
        raise ValueError(f"dump_results: the ring degree must be a power of two below N = {n}, got {ring}")
    if need > r:
        raise ValueError(f"dump_results: 2 G period = {need} coefficients do not fit the ring degree {r}")
    if not accepted(r):
        raise ValueError(f"dump_results: ring too small for this modulus (R = {r} admits log2(Q0 P') <= {max_log_modulus(r)} at 128 "
                         f"bits, one special prime gives {bits:.1f}; insecure_ok lifts this for test rings)")
    return r


def dump_results(ctx, cts, period=None, ring=None, insecure_ok=False):
    """(array, meta): the pack's residues [2][nl(0)][N] uint32 (ctx.engine.export) and a plain, json-serialisable dict
    -- members T, G, period, slots, and each member's layout tag and value_dtype tag (None: untagged / absent).

    ring: a ring degree R (a power of two, 2 G period <= R < N) or "auto" (the smallest the 128-bit
    gate accepts): the pack is ring-switched (ctx.ring_switch) and travels as the (2, 2, R) uint32 array of its
    coefficient-form residues mod q0, q1 under the subring secret; meta gains ring, moduli (q0, q1), scale (delta_0) and
    special (the special primes P' of the ring key: ring_switch_bound's input).  insecure_ok lifts the gate for small
    test rings.  ValueError: a ring that is no power of two below N, 2 G period > ring, a ring the gate refuses"""
    cts = list(cts)
    z = pack_results(ctx, cts, period)
    G, per = z.pack
    meta = dict(members=len(cts), G=int(G), period=int(per), slots=int(ctx.engine.slot_count),
                present=[c is not None for c in cts],
                layouts=[None if c is None else _layout_tag(c) for c in cts],
                value_dtypes=[None if c is None else getattr(c, "value_dtype", None) for c in cts])
    if ring is None:
        return ctx.engine.export(z), meta
    eng = ctx.engine
    r = _choose_ring(eng, G, per, ring, bool(insecure_ok))
    fn = getattr(ctx, "ring_switch", None) or getattr(eng, "ring_switch", None)
    if fn is None:
        raise RuntimeError("dump_results: this engine has no aesfhe_ring_switch entry point (rebuild the library); "
                           "there is no host fallback for switching ciphertexts")
    array = fn(z, r, bool(insecure_ok))
    mod = [int(m) for m in eng.moduli()]
    n_sp = int(eng.ksk_words(eng.ring_key_tag(r))) // (2 * RING_KEY_DIGITS * 2 * int(eng.slot_count)) - 2   # rows per polynomial - 2
    meta.update(ring=r, moduli=mod[:2], scale=float(eng.scales()[0]), special=mod[int(eng.n_q):int(eng.n_q) + n_sp])
    return array, meta


# ---------------------------------------------------------------- ring-switched packs
RING_KEY_DIGITS = 2       # csrc/engine.hip kRingDigits: q0 and q1 a digit each
KEY_ERROR_SIGMA = float(np.sqrt(10.5))   # k_sample_small's centred binomial of 2 x 21 bits: variance 42 / 4
_MAX_LOG_MODULUS = {1024: 27, 2048: 54, 4096: 109, 8192: 218, 16384: 438, 32768: 881, 65536: 1772}


def max_log_modulus(ring: int) -> int:
    """the largest log2 of the modulus for a ternary secret of dimension `ring` at 128 bits classical (the Homomorphic
    Encryption Standard's table; csrc/engine.hip ring_max_log_modulus); 0 below 1024: no modulus is admitted"""
    return _MAX_LOG_MODULUS.get(int(ring), 0)


def ring_switch_bound(meta, coefficient: bool = False) -> float:
    """E_R: the analytic worst-case slot error the level-0 key switch to s_R adds.  Per coefficient:
    the gadget term 2 digits x q_max x N terms x 6 sigma / P' plus the ModDown's rounding (1 + ||s_R||_1) / 2 with
    ||s_R||_1 <= R; divided by the scale and summed over the R coefficients of the small ring for a slot.
    coefficient=True: the per-coefficient bound itself (integers mod q0 q1).  meta: dump_results' (ring, slots, moduli,
    special, scale)"""
    r, n = int(meta["ring"]), 2 * int(meta["slots"])
    q_max = float(max(int(m) for m in meta["moduli"]))
    p = 1.0
    for m in meta["special"]:
        p *= float(m)
    coef = RING_KEY_DIGITS * q_max * n * 6.0 * KEY_ERROR_SIGMA / p + (1.0 + r) / 2.0
    return coef if coefficient else r * coef / float(meta["scale"])


def ring_phase(array, secret, moduli) -> list:
    """the phase c0' + c1' s_R in Z[X] / (X^R + 1) per limb, reduced to [0, q): an exact negacyclic product by signed
    shifts over the nonzeros of the ternary s_R.  int64 cannot overflow: each of the at most R + 1 <= 2^16 + 1 terms is a
    residue below 2^30, so every partial sum lies within 2^47"""
    a = np.asarray(array)
    if a.ndim != 3 or a.shape[0] != 2 or a.shape[1] != len(moduli):
        raise ValueError(f"a ring-switched pack is a (2, {len(moduli)}, ring) array, got shape {a.shape}")
    r = a.shape[2]
    s = np.asarray(secret, np.int64).reshape(-1)
    if s.shape[0] != r or np.abs(s).max(initial=0) > 1:
        raise ValueError(f"the subring secret has {r} ternary coefficients, got shape {s.shape}")
    out = []
    for l, q in enumerate(moduli):
        c1 = a[1, l].astype(np.int64)
        acc = a[0, l].astype(np.int64)
        for i in np.flatnonzero(s):
            # X^i c1: coefficient j <- c1[j - i], negated where it wrapped
            sh = np.concatenate((-c1[r - i:], c1[:r - i])) if i else c1
            acc = acc + sh if s[i] > 0 else acc - sh
        out.append(np.mod(acc, int(q)))
    return out


def crt_centred(residues, moduli) -> np.ndarray:
    """the centred integers mod q0 q1 (object dtype: exact) of a two-limb residue pair"""
    q0, q1 = int(moduli[0]), int(moduli[1])
    x0, x1 = residues[0].astype(object), residues[1].astype(object)
    inv = pow(q0, -1, q1)
    x = x0 + q0 * (((x1 - x0) * inv) % q1)        # in [0, q0 q1)
    Q = q0 * q1
    return np.where(x > Q // 2, x - Q, x)


def small_ring_slots(coeffs) -> np.ndarray:
    """the R / 2 slots of a real coefficient vector of the ring of degree R: slot t = sum_j c_j w^(j 5^t), w = exp(i pi / R)
    -- the big ring's slot t for a polynomial of Z[X^k] (zeta^k = w, and 5^t has period R / 2 mod 2 R)"""
    c = np.asarray(coeffs, np.float64)
    r = c.shape[0]
    # the odd powers of w all at once: c_j w^j, then an FFT of length R gives sum_j c_j w^(j (2 m + 1)) at index m
    tw = np.exp(1j * np.pi * np.arange(r) / r)
    ev = np.fft.ifft(c * tw) * r                      # ev[m] = sum_j c_j w^j exp(2 pi i j m / R) = p(w^(2 m + 1))
    e = slot_exponents(r // 2) if r >= 2 else np.ones(1, np.int64)
    return ev[((e % (2 * r)) - 1) // 2]


def ring_decrypt(array, secret, meta) -> np.ndarray:
    """Client side of a ring-switched pack, numpy only: phase per limb, CRT to the centred integer mod q0 q1, division by
    the scale, the R / 2 slots of the small ring, tiled to the big ring's slot count"""
    r, sc = int(meta["ring"]), int(meta["slots"])
    if r < 2 or r & (r - 1) or r // 2 > sc:
        raise ValueError(f"result pack: a ring degree of {r} does not belong to {sc} slots")
    a = np.asarray(array)
    if a.shape != (2, 2, r):
        raise ValueError(f"result pack: a ring-switched pack of degree {r} is a (2, 2, {r}) array, got shape {a.shape}")
    moduli = [int(m) for m in meta["moduli"]]
    if (a >= np.asarray(moduli, np.uint64).reshape(1, 2, 1)).any():
        raise ValueError("result pack: a residue not below its modulus")
    x = crt_centred(ring_phase(a, secret, moduli), moduli)
    z = small_ring_slots(x.astype(np.float64) / float(meta["scale"]))
    return np.tile(z, sc // (r // 2))


def check_meta(meta, sc: int) -> None:
    T, G, per = int(meta["members"]), int(meta["G"]), int(meta["period"])
    if int(meta["slots"]) != sc:
        raise ValueError(f"result pack: made for {meta['slots']} slots, this context has {sc}")
    if G != group_size(T):
        raise ValueError(f"result pack: G = {G} does not belong to {T} members")
    _check(G, per, sc)
    if len(meta["layouts"]) != T or len(meta["value_dtypes"]) != T:
        raise ValueError("result pack: one layout and one value_dtype entry per member expected")


def unpack_results(ctx, array, meta):
    """Client side: load_ct(level 0, check=True) -> ctx.decrypt -> split_slots; the T members' full-length slot vectors
    (period tiled), which the existing slot decoders (StateEncoder.decode_slots / values_from_slots) take unchanged"""
    sc = int(ctx.engine.slot_count)
    check_meta(meta, sc)
    if meta.get("ring") is not None:
        # a ring-switched pack: decrypted in the small ring, in numpy, under s_R ("no secret key" on an
        # evaluation-only context); its slots tiled are the big ring's
        if 2 * int(meta["G"]) * int(meta["period"]) > int(meta["ring"]):
            raise ValueError(f"result pack: G * period = {int(meta['G']) * int(meta['period'])} slots do not fit the ring degree {meta['ring']}")
        z = ring_decrypt(array, ctx.ring_secret(int(meta["ring"])), meta)
        return split_slots(z, int(meta["G"]), int(meta["period"]))[:int(meta["members"])]
    z = ctx.decrypt(load_ct(ctx, np.asarray(array), 0, None, check=True))
    return split_slots(z, int(meta["G"]), int(meta["period"]))[:int(meta["members"])]
