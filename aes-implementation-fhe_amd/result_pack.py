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


def dump_results(ctx, cts, period=None):
    """(array, meta): the pack's residues [2][nl(0)][N] uint32 (ctx.engine.export) and a plain, json-serialisable dict
    -- members T, G, period, slots, and each member's layout tag and value_dtype tag (None: untagged / absent)"""
    cts = list(cts)
    z = pack_results(ctx, cts, period)
    G, per = z.pack
    meta = dict(members=len(cts), G=int(G), period=int(per), slots=int(ctx.engine.slot_count),
                present=[c is not None for c in cts],
                layouts=[None if c is None else _layout_tag(c) for c in cts],
                value_dtypes=[None if c is None else getattr(c, "value_dtype", None) for c in cts])
    return ctx.engine.export(z), meta


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
    z = ctx.decrypt(load_ct(ctx, np.asarray(array), 0, None, check=True))
    return split_slots(z, int(meta["G"]), int(meta["period"]))[:int(meta["members"])]
