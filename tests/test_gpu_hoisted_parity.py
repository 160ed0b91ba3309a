"""The hoisted MACs and the batched key switch, bit for bit against the CPU oracle, with every operand chosen.

rot_pt_sum / rot_pt_affine (k_rot_mask_mac<ND, FILL>), galois_multi / rotate_multi / conjugate_many (k_key_inner_multi,
k_automorph_multi, the batched ModDown) and mul_pt_sum (k_mul_poly_sum) were checked only against decrypted values, against
digests of the engine's own earlier output, or with generated keys and uniform data.  Here:

* the engine is evaluation-only and every key is imported (tests/helpers/keyswitch_shapes_probe.py): `top` keys are
  q - 1 in every word under every tag, `corners` keys are a DIFFERENT array per tag, seeded by the tag, so a kernel
  that read member m's digits against member m''s key cannot pass;
* the plaintexts encode to known integer polynomials (tests/helpers/edge_patterns.py pt_top / pt_impulse / pt_small;
  exactness asserted on the CPU in tests/test_oracle_hoisted.py and on the engine's encoder in
  test_engine_encodes_patterns_exactly below), so the masks' residues on every Q and P row are NTT(m);
* the model of a masked rotation sum is written with the oracle's three exported steps (oracle/ckks_cpu.py modup,
  key_inner, moddown), because the sum multiplies and adds in Q P between the inner product and the ModDown:
      acc_j  = sum_i P_ji (.) inner(ModUp(c1), key_i, g_i)                       over Q P
      out_j  = ModDown(acc_j) + (sum_i P_ji (.) sigma_gi(c0) + fill_j,  sum_{step 0} P_ji (.) c1)
  then the oracle's rescale, which export settles;
* with everything at `top` and 16 terms the inner digit sums and the Q-side sum of k_rot_mask_mac sit at their bounds;
  the Q P-side sums take the REDUCED inner product, so they are driven by keys of 1 on digit 0 instead (DESIGN.md
  §5b); the closed forms are asserted beside the model.

Sets: A, B, C, D of keyswitch_shapes_probe (1, 2, 10, 19 digits at the top level) plus F and G (3 and 4 digits): the four
templated digit bodies and the run-time loop with one and two inner folds; E (N = 2^16) once.  Every comparison is
np.array_equal; no tolerance anywhere."""
import contextlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

import edge_patterns as ep  # noqa: E402
import keyswitch_shapes_probe as ks  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = dict(ks.SETS, F=(13, 10, 3), G=(13, 10, 4))  # F: alpha 4, 3 digits at the top; G: alpha 3, 4 digits
N_TERMS = 16                                        # kRotMacMax
CT_KINDS = ("top", "corners", "uniform")
PT_KINDS = ("top", "impulse", "small")


def rot_steps(sc):
    """16 steps with 16 different keys, none zero modulo the slot count: negative ones, one at slot_count + 3 (the same
    rotation as 3 would be, so 3 itself is left out) and one beyond 2 slot_count"""
    return [1, -1, 2, sc + 3, -5, 7, 2 * sc + 11, 16, -16, 33, sc // 2, -sc // 4, 100, sc - 2, 6, -9]


class Pat:
    """a plaintext of known residues: slots z (built for `scale`), the integer polynomial m, the engine's handle"""

    def __init__(self, rig, kind, scale, seed=0):
        O = rig.O
        self.z, self.m = {"top": lambda: ep.pt_top(O, scale), "impulse": lambda: ep.pt_impulse(O, scale, O.n // 2 + 1 + seed),
                          "small": lambda: ep.pt_small(O, scale, 1000 + seed)}[kind]()
        self.h = rig.E.encode(self.z)
        assert self.h.const is None


class Rig:
    def __init__(self, name, key_kind):
        from mi355x_ckks import Engine
        from oracle.ckks_cpu import OracleParams
        log_n, L, dnum = SETS[name]
        self.name, self.key_kind = name, key_kind
        self.O = O = OracleParams(log_n=log_n, max_level=L, dnum=dnum, seed=ks.SEED)
        self.E = E = Engine.evaluation_only(prng_key=bytes(range(32)), log_n=log_n, max_level=L, dnum=dnum, allow_insecure=True,
                                            enc_nonce=1, lazy=False, defer_calls=False)
        E.set_low_p(False)
        assert np.array_equal(E.moduli(), O.moduli) and np.array_equal(E.scales(), O.deltas)
        assert (E.alpha, E.n_p, E.n_ks) == (O.alpha, O.n_p, O.n_ks)
        E.import_pk(np.zeros((2, E.n_q, E.n), np.uint32))  # import_ct asks for a public key; none is used
        self.sc = O.slot_count
        self.steps = rot_steps(self.sc)
        self.g_conj = O.galois_conj
        rots = [O.galois_rotate(s) for s in self.steps]
        assert len(set(rots)) == N_TERMS and 1 not in rots and all(E.galois_rotate(s) == g for s, g in zip(self.steps, rots))
        self.tags = sorted({0, self.g_conj, 4 * O.n + self.g_conj, *rots})  # 0: relinearisation; 4N + g: sigma_g(s)^2 -> s
        self._keys = {}
        for g in self.tags:
            E.import_ksk(g, -1, self.key(g))
        self._pats = {}

    def key(self, g):
        """the key imported under tag g: `top` is one array; `corners` is seeded by the tag, different under each"""
        if g not in self._keys:
            if self.key_kind == "top":
                if "top" not in self._keys:
                    self._keys["top"] = ks.make_key(self.O, "top")
                self._keys[g] = self._keys["top"]
            elif self.key_kind == "unit":  # 1 in every word of digit 0, zero elsewhere: the inner product is digit 0 itself
                if "unit" not in self._keys:
                    k = np.zeros_like(ks.make_key(self.O, "top"))
                    k[0] = 1
                    self._keys["unit"] = k
                self._keys[g] = self._keys["unit"]
            else:
                self._keys[g] = ks.make_key(self.O, "corners", seed=int(g) * 64 + 1)
        return self._keys[g]

    def mask_scale(self, lv):
        return ep.pt_scale(self.E.scales(), self.E.moduli(), lv)

    def fill_scale(self, lv):
        """the product scale of an output owing its rescale (csrc/engine.hip raw_scale(l, 1)): delta[l-1] q_{l+1}"""
        return float(self.E.scales()[lv - 1]) * float(self.E.moduli()[lv + 1])

    def mask(self, lv, kind, seed=0):
        k = ("m", lv, kind, seed)
        if k not in self._pats:
            self._pats[k] = Pat(self, kind, self.mask_scale(lv), seed)
        return self._pats[k]

    def fill(self, lv, kind, seed=0):
        k = ("f", lv, kind, seed)
        if k not in self._pats:
            self._pats[k] = Pat(self, kind, self.fill_scale(lv), 500 + seed)
        return self._pats[k]

    def ct(self, lv, kind, seed):
        q = self.O.moduli[: self.O.nl(lv)]
        f = {"top": lambda s: ep.top(q, self.O.n), "corners": lambda s: ep.corners(q, self.O.n, s),
             "uniform": lambda s: ep.uniform(q, self.O.n, s)}[kind]
        return np.stack([f(seed), f(seed + 1)])

    def levels(self):
        return sorted({self.O.L, self.O.L // 2, 1}, reverse=True)


RIGS = [(s, k) for s in "ABCDFG" for k in ("top", "corners")]


@pytest.fixture(scope="module", params=RIGS, ids=lambda p: f"{p[0]}_{p[1]}")
def rig(request):
    r = Rig(*request.param)
    yield r
    del r.E


@contextlib.contextmanager
def own_rig(name, key_kind):
    """a rig of one test's own: its engine goes whether the test passes or fails"""
    r = Rig(name, key_kind)
    try:
        yield r
    finally:
        del r.E


# ----------------------------------------------------------------------------------------- the model
def rot_sum_model(rig, lv, ct, steps, masks, fills, np_=None, key=None):
    """[out_j] of rot_pt_sum / rot_pt_affine (see the module docstring), exported: [2][nl - 1][N] each.
    masks[j][i]: a Pat or None; fills[j]: a Pat or None; np_: the special primes (None: the full basis); key(g): the key of
    a tag (default: the rig's full keys)"""
    O = rig.O
    key = key or rig.key
    nl = O.nl(lv)
    np_eff = O.n_p if np_ is None else np_
    limbs = list(range(nl)) + list(range(O.n_q, O.n_q + np_eff))
    qe = O.ext_moduli(lv, np_).astype(np.uint64)[:, None]
    qq = O.limbs_mod(nl)
    c0, c1 = ct
    ext, inner, sig0, ntt_m = None, {}, {}, {}
    outs = []
    for ms, fill in zip(masks, fills):
        acc = np.zeros((2, nl + np_eff, O.n), np.uint64)
        a0, a1 = np.zeros((nl, O.n), np.uint64), np.zeros((nl, O.n), np.uint64)
        rotated = False
        for i, st in enumerate(steps):
            if ms[i] is None:
                continue
            if id(ms[i]) not in ntt_m:
                ntt_m[id(ms[i])] = ep.poly_ntt(O, ms[i].m, limbs).astype(np.uint64)
            P = ntt_m[id(ms[i])]
            if st % rig.sc == 0:  # no key switch: the term stays on the Q limbs, c1 included
                a0 = (a0 + P[:nl] * c0 % qq) % qq
                a1 = (a1 + P[:nl] * c1 % qq) % qq
                continue
            g = O.galois_rotate(st)
            if i not in inner:
                if ext is None:
                    ext = O.modup(lv, c1, np_)
                inner[i] = O.key_inner(lv, ext, c1, key(g), g, np_).astype(np.uint64)
                sig0[i] = O.automorph(lv, g, c0[None])[0].astype(np.uint64)
            acc = (acc + P[None] * inner[i] % qe) % qe
            a0 = (a0 + P[:nl] * sig0[i] % qq) % qq
            rotated = True
        if fill is not None:
            a0 = (a0 + ep.poly_ntt(O, fill.m, range(nl))) % qq
        if rotated:
            out = O.moddown(lv, acc.astype(np.uint32), a0.astype(np.uint32), a1.astype(np.uint32), np_)
        else:
            out = np.stack([a0, a1]).astype(np.uint32)
        outs.append(O.rescale(lv, out))
    return outs


def run_rot(rig, lv, ct, steps, masks, fills):
    E = rig.E
    h = [[None if p is None else p.h for p in ms] for ms in masks]
    c = E.import_ct(ct, lv)
    if any(f is not None for f in fills):
        outs = E.rot_pt_affine(c, steps, h, [None if f is None else f.h for f in fills])
    else:
        outs = E.rot_pt_sum(c, steps, h)
    return [E.export(o) for o in outs]


def check_rot(rig, lv, ct, steps, masks, fills=None, what=""):
    fills = fills or [None] * len(masks)
    got = run_rot(rig, lv, ct, steps, masks, fills)
    want = rot_sum_model(rig, lv, ct, steps, masks, fills)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (rig.name, rig.key_kind, lv, what, j)
    return got


# ------------------------------------------------------------------------------- the engine's encoder
def test_engine_encodes_patterns_exactly(rig):
    """once per rig: the engine's own encoder maps every pattern to its polynomial.  The ciphertext (NTT(1), 0) times
    the plaintext is the plaintext's Q rows; exported, the settled product is rescale(NTT(m), 0) -- so a failure of
    the sums below is never an encoder disagreement"""
    E, O = rig.E, rig.O
    for lv in rig.levels():
        nl = O.nl(lv)
        one = np.stack([np.ones((nl, O.n), np.uint32), np.zeros((nl, O.n), np.uint32)])
        for kind in PT_KINDS:
            p = rig.mask(lv, kind)
            got = E.export(E.multiply(E.import_ct(one, lv), p.h))
            want = O.rescale(lv, np.stack([ep.poly_ntt(O, p.m, range(nl)), np.zeros((nl, O.n), np.uint32)]))
            assert np.array_equal(got, want), (lv, kind)


# --------------------------------------------------------------------------- rot_pt_sum / rot_pt_affine
def test_rot_pt_sum_all_top_at_the_bound(rig):
    """16 terms, ciphertext, masks and (on the `top` rigs) keys all q - 1.  The accumulators of k_rot_mask_mac at their
    bounds: the inner sums s0 / s1 hold 8 products (q-1)^2 beside a folded value before each inner fold (19 digits
    without it: 19 (q-1)^2 > 2^64 on the primes above 0.918 2^30), the Q-side sum a0 holds 8 products (q-1)^2 beside a
    folded value before the outer fold at i = 8 and again at the end.  The P-side sums p0 / p1 take u (q-1) with u the
    REDUCED inner product, which is only nd here; test_rot_pt_sum_unit_keys_at_the_bound drives them.

    Closed form (top keys): ModUp of -1 is -1 on every row (the centred conversion of a digit whose value is -1),
    the automorphism of the constant -1 is -1, so each inner product is nd (-1)(-1) = nd on every row of Q P, both
    halves; times the mask -1 and summed over n terms: -n nd on every row of Q P -- the small integer -n nd, which
    the ModDown by P rounds to 0.  The addends: c0 is the constant -1, so a0 = n (-1)(-1) = n; a1 = 0 (no step-0
    term).  Before the rescale the result is (n, 0) in every NTT word, the NTT form of the constant n; the rescale
    rounds n / q_l to 0: the settled result is all zeros"""
    n = N_TERMS
    for lv in rig.levels():
        ct = rig.ct(lv, "top", 0)
        m = rig.mask(lv, "top")
        got = check_rot(rig, lv, ct, rig.steps, [[m] * n], what="all top")
        if rig.key_kind == "top":
            assert not got[0].any(), lv
            # the unsettled closed form, through the model's own last steps: ModDown(-n nd) + (n, 0) == (n, 0)
            O = rig.O
            nl, nd = O.nl(lv), O.ks_digits(lv)
            qe = O.ext_moduli(lv).astype(np.int64)[:, None]
            acc = np.broadcast_to((-n * nd) % qe, (2, len(qe), O.n)).astype(np.uint32)
            a0 = np.full((nl, O.n), n, np.uint32)
            pre = O.moddown(lv, acc, a0, None)
            assert (pre[0] == n).all() and not pre[1].any(), lv
            assert not O.rescale(lv, pre).any(), lv


@pytest.mark.parametrize("name", ["A", "D"])
def test_rot_pt_sum_unit_keys_at_the_bound(name):
    """the P-side sums p0 / p1 at their bound: they take u (.) mask with u the reduced inner product, so they fill
    only when u is large.  Keys of 1 in every word of digit 0 and 0 elsewhere make u = the extended digit 0 of c1
    = -1 on every row; with masks -1 every one of the 16 products is (q-1)^2: 8 of them beside a folded value before
    the fold at i = 8 and at the end.  Closed form: acc = 16 (-1)(-1) = 16 on every row of Q P, both halves, which the
    ModDown rounds to 0; a0 = 16, a1 = 0; settled: all zeros.  1 digit (set A) and 19 (set D)"""
    with own_rig(name, "unit") as r:
        for lv in r.levels():
            got = check_rot(r, lv, r.ct(lv, "top", 0), r.steps, [[r.mask(lv, "top")] * N_TERMS], what="unit keys")
            assert not got[0].any(), lv


def test_rot_pt_sum_term_counts_and_absent_terms(rig):
    """1, 8, 9 and 16 terms (the outer fold sits at i = 8); an absent term at i = 8 and one at i = 0 (the fold is
    written before the `continue`); operands and masks of every kind"""
    for lv in rig.levels():
        top_level = lv == rig.O.L
        for n in (1, 8, 9, 16):
            ck = CT_KINDS[(n + lv) % 3] if not top_level else "corners"
            ct = rig.ct(lv, ck, 10 + n)
            ms = [rig.mask(lv, PT_KINDS[(i + n) % 3], i % 4) for i in range(n)]
            check_rot(rig, lv, ct, rig.steps[:n], [ms], what=f"{n} terms")
        if not top_level:
            continue
        for ck in CT_KINDS:
            ct = rig.ct(lv, ck, 20)
            ms = [rig.mask(lv, PT_KINDS[i % 3], i % 4) for i in range(N_TERMS)]
            ms[8] = None
            ms[0] = None
            check_rot(rig, lv, ct, rig.steps, [ms], what=f"absent 0 and 8, {ck}")
        top = [rig.mask(lv, "top")] * N_TERMS
        top[8] = None
        check_rot(rig, lv, rig.ct(lv, "top", 0), rig.steps, [top], what="absent 8, all top")


def test_rot_pt_sum_two_outputs_step0_and_fills(rig):
    """two outputs sharing some terms and not others; a step-0 term alone (no key switch, no outp); step 0 -- written
    as 0, as slot_count and as -2 slot_count -- mixed with rotated terms; fills on one output, on both, on none"""
    sc = rig.sc
    for lv in rig.levels():
        M = lambda k, s=0: rig.mask(lv, k, s)  # noqa: E731
        F = lambda k, s=0: rig.fill(lv, k, s)  # noqa: E731
        ct = rig.ct(lv, "corners", 30)
        # a step-0 term alone, one output and two
        check_rot(rig, lv, ct, [0], [[M("small")]], what="step 0 alone")
        check_rot(rig, lv, ct, [sc], [[M("impulse")], [M("top")]], what="step slot_count alone, two outputs")
        # mixed: steps 0 / sc / -2 sc are unrotated terms, the rest rotate
        steps = [0, 3 + sc, -5, sc, 7, -2 * sc, 16, 1, -1]
        o0 = [M("small", 1), M("top"), None, M("impulse"), M("small", 2), None, M("top"), M("impulse", 1), M("small", 3)]
        o1 = [None, M("top"), M("small", 1), None, M("small", 2), M("impulse", 2), None, M("impulse", 1), None]
        steps[1] = rig.steps[3]  # sc + 3: a key the rig holds
        for ck in CT_KINDS if lv == rig.O.L else ("corners",):
            c = rig.ct(lv, ck, 31)
            check_rot(rig, lv, c, steps, [o0, o1], what=f"two outputs, {ck}")
            check_rot(rig, lv, c, steps, [o0, o1], [F("small"), None], what=f"fill on output 0, {ck}")
            check_rot(rig, lv, c, steps, [o0, o1], [F("top"), F("impulse")], what=f"fills on both, {ck}")
        # the second output unrotated only: its Q-side sums are its result while the first goes through the ModDown
        check_rot(rig, lv, ct, [0, 1, -1], [[M("top"), M("small"), M("impulse")], [M("small", 1), None, None]],
                  [None, F("small", 1)], what="second output unrotated, filled")
        # rot_pt_affine with every fill None is rot_pt_sum's launch
        h = [[p.h for p in (M("top"), M("small"))]]
        a = rig.E.export(rig.E.rot_pt_affine(rig.E.import_ct(ct, lv), [1, 2], h, [None])[0])
        assert np.array_equal(a, rig.E.export(rig.E.rot_pt_sum(rig.E.import_ct(ct, lv), [1, 2], h)[0])), lv


def test_rot_pt_sum_low_p():
    """set A under set_low_p(True) at a level below alpha limbs: one digit over nl + 1 special primes, that level's own
    key under each tag (as test_refuses_17_special_primes imports its reduced-basis key); the model runs the same
    wrappers at nl + 1 special primes"""
    with own_rig("A", "corners") as r:
        E, O = r.E, r.O
        E.set_low_p(True)
        lv = 5
        nl = O.nl(lv)
        assert nl < O.alpha and E.ks_special_primes(lv) == nl + 1
        qk = O.ext_moduli(lv, nl + 1)
        keys = {}
        for s in r.steps:
            g = O.galois_rotate(s)
            keys[g] = np.stack([ep.corners(qk, O.n, 2 * g), ep.uniform(qk, O.n, 2 * g + 1)])
            E.import_ksk(g, lv, keys[g])
        for ck, pk in (("top", "top"), ("corners", "small"), ("uniform", "impulse")):
            ct = r.ct(lv, ck, 40)
            ms = [r.mask(lv, pk if i % 2 else "top", i % 3) for i in range(N_TERMS)]
            ms[8] = None
            fills = [r.fill(lv, "small")]
            got = run_rot(r, lv, ct, r.steps, [ms], fills)
            want = rot_sum_model(r, lv, ct, r.steps, [ms], fills, np_=nl + 1, key=keys.__getitem__)
            assert np.array_equal(got[0], want[0]), (ck, pk)


def test_rot_pt_sum_n65536():
    """set E, the N = 2^16 kernels: one level, 16 terms, `top` everywhere; the model and the closed form (all zeros,
    see test_rot_pt_sum_all_top_at_the_bound)"""
    with own_rig("E", "top") as r:
        lv = r.O.L // 2
        m = r.mask(lv, "top")
        got = check_rot(r, lv, r.ct(lv, "top", 0), r.steps, [[m] * N_TERMS], what="E all top")
        assert not got[0].any()


# ------------------------------------------------------------- galois_multi / rotate_multi / conjugate_many
def galois_model(rig, lv, a, g):
    """rotate's model: automorphism, key switch of the permuted c1 under the tag's key, add the permuted c0"""
    O = rig.O
    if g == 1:
        return a
    x = O.automorph(lv, g, a)
    want = O.keyswitch(lv, x[1], rig.key(g))
    want[0] = ((want[0].astype(np.uint64) + x[0]) % O.limbs_mod(O.nl(lv))).astype(np.uint32)
    return want


def test_galois_multi_bitexact(rig):
    """one source three times under different elements, unrelated sources in shuffled order (the gathered c1), rotations
    and conjugations mixed, the identity, sources at two levels, 13 items (a second chunk), and on sets C and D three and
    more distinct sources at the top level (sources x digits above 24: the ModUp splits).  On the `corners` rigs every
    tag has its own key: an item switched under another item's key fails here and nowhere else"""
    E, O = rig.E, rig.O
    top, low = O.L, O.L // 2
    rot = [O.galois_rotate(s) for s in rig.steps]
    conj = rig.g_conj
    src = {k: (rig.ct(top, CT_KINDS[i % 3], 50 + 2 * i), top) for i, k in enumerate("abcde")}
    src["l"] = (rig.ct(low, "corners", 70), low)
    src["m"] = (rig.ct(low, "top", 72), low)
    items = [("a", rot[0]), ("a", rot[4]), ("a", conj), ("b", conj), ("a", 1), ("l", rot[2]), ("d", rot[1]), ("m", conj),
             ("c", rot[5]), ("e", rot[0]), ("b", rot[7]), ("l", 1), ("c", rot[0])]
    h = {k: E.import_ct(a, lv) for k, (a, lv) in src.items()}
    outs = E.galois_multi([(h[k], g) for k, g in items])
    assert len(outs) == len(items)
    for (k, g), o in zip(items, outs):
        a, lv = src[k]
        assert o.level == lv
        assert np.array_equal(E.export(o), galois_model(rig, lv, a, g)), (k, g)
    # rotate_multi: steps, not elements -- one at slot_count + 3
    st = [(("a"), rig.steps[3]), ("b", rig.steps[1]), ("a", rig.steps[6])]
    for (k, s), o in zip(st, E.rotate_multi([(h[k], s) for k, s in st])):
        assert np.array_equal(E.export(o), galois_model(rig, top, src[k][0], O.galois_rotate(s))), (k, s)


def test_galois_multi_same_source_distinct_keys(rig):
    """ONE source, 8 members in one chunk, all `top` but the keys: with a different key under every tag the 8 results
    must be the 8 models; with the key of member m' under member m's read they would not be.  (On a `top` rig every
    tag holds the same array and only the automorphisms distinguish the members.)"""
    E, O = rig.E, rig.O
    lv = O.L
    a = rig.ct(lv, "top", 0)
    gs = [O.galois_rotate(s) for s in rig.steps[:7]] + [rig.g_conj]
    c = E.import_ct(a, lv)
    got = [E.export(o) for o in E.galois_multi([(c, g) for g in gs])]
    want = [galois_model(rig, lv, a, g) for g in gs]
    for g, x, w in zip(gs, got, want):
        assert np.array_equal(x, w), g
    if rig.key_kind == "corners":  # the automorphism of the constant -1 is itself: only the key tells the members apart
        assert len({w.tobytes() for w in want}) == len(gs)


def test_conjugate_many_bitexact(rig):
    """conjugate_many on canonical inputs (galois_many: one batched key switch), and on one lazy product: under
    set_lazy(True) multiply(x, y, "rlk") stays the 3-polynomial tensor owing its relinearisation and its rescale, and
    its conjugation reads sigma(d1) under the key of tag g and sigma(d2) under the key of tag 4N + g as two sources
    summed in Q P before ONE ModDown adding sigma(d0); export settles the owed rescale.  (With chosen keys the
    relinearised, rescaled product conjugated is a different array: a key here is a key only in shape.)"""
    E, O = rig.E, rig.O
    g = rig.g_conj
    for lv in (O.L, 1):
        srcs = [rig.ct(lv, CT_KINDS[i % 3], 80 + 2 * i) for i in range(3)]
        outs = E.conjugate_many([E.import_ct(a, lv) for a in srcs])
        for a, o in zip(srcs, outs):
            assert np.array_equal(E.export(o), galois_model(rig, lv, a, g)), lv
    # the two sources share one ModUp launch of at most 24 conversion groups (modup: sources x digits <= kMaxConvGroups):
    # set D's upper levels (2 x 13 .. 19 digits) are refused on the host, as test_refuses_25_digits' shape is
    fits = max(lv for lv in range(1, O.L + 1) if 2 * O.ks_digits(lv) <= 24)
    if fits < O.L:
        x = rig.ct(O.L, "corners", 90)
        E.set_lazy(True)
        try:
            prod = E.multiply(E.import_ct(x, O.L), E.import_ct(x, O.L), "rlk")
            with pytest.raises(RuntimeError, match="keyswitch: digit too large"):
                E.conjugate_many([prod])
        finally:
            E.set_lazy(False)
    for lv in (fits, 1):
        for ck in CT_KINDS:
            x, y = rig.ct(lv, ck, 90), rig.ct(lv, ck, 92)
            E.set_lazy(True)
            try:
                prod = E.multiply(E.import_ct(x, lv), E.import_ct(y, lv), "rlk")
                got = E.export(E.conjugate_many([prod])[0])
            finally:
                E.set_lazy(False)
            t = O.automorph(lv, g, O.tensor(lv, x, y))
            qe = O.ext_moduli(lv).astype(np.uint64)[:, None]
            acc = (O.key_inner(lv, O.modup(lv, t[1]), t[1], rig.key(g)).astype(np.uint64)
                   + O.key_inner(lv, O.modup(lv, t[2]), t[2], rig.key(4 * O.n + g))) % qe
            want = O.rescale(lv, O.moddown(lv, acc.astype(np.uint32), t[0], None))
            assert np.array_equal(got, want), (lv, ck)


# ----------------------------------------------------------------------------------------- mul_pt_sum
def mul_pt_sum_model(rig, l, cts, pats):
    """sum_i NTT(m_i) (.) ct_i on the Q limbs of level l -- an operand above l first takes the exact level drop
    (OracleEngine.level_down's arithmetic) -- then rescale"""
    O = rig.O
    nl = O.nl(l)
    qq = O.limbs_mod(nl)
    acc = np.zeros((2, nl, O.n), np.uint64)
    for (a, lv), p in zip(cts, pats):
        if lv != l:
            c = int(round(O.deltas[l] * float(O.moduli[l + 2]) / O.deltas[lv]))
            a = O.rescale(l + 1, O.mul_limb_consts(O.const_residues(c, l + 3), np.ascontiguousarray(a[:, : l + 3])))
        acc = (acc + a.astype(np.uint64) * ep.poly_ntt(O, p.m, range(nl)).astype(np.uint64)[None] % qq) % qq
    return acc.astype(np.uint32)


def test_mul_pt_sum_bitexact(rig):
    """1, 8 and 9 pairs: 8 is kMaxMembers, the most one k_mul_poly_sum launch sums (8 products in a u64, no fold), and 9 is refused on the host ("1..8
    pairs", documented in mul_pt_sum's docstring) with the engine left usable.  One operand two levels above the
    others takes the exact drop.

    Closed form at 8 pairs, `top` on both sides: every product is (-1)(-1) = 1, so the sum is 8 in every word of the
    NTT form on every Q limb -- the NTT form of the constant polynomial 8.  The rescale divides the constant 8 by q_l
    with rounding: 0.  The settled result is all zeros; the unsettled sum is asserted on the model's side."""
    E, O = rig.E, rig.O
    for l in sorted({O.L - 2, O.L // 2, 1}, reverse=True):
        for n in (1, 8):
            for ck in CT_KINDS:
                cts = [(rig.ct(l, ck, 100 + 2 * i), l) for i in range(n)]
                if n == 8:
                    cts[3] = (rig.ct(l + 2, ck, 120), l + 2)  # the exact level drop
                pats = [rig.mask(l, "top" if ck == "top" else PT_KINDS[i % 3], i % 4) for i in range(n)]
                pre = mul_pt_sum_model(rig, l, cts, pats)
                got = E.export(E.mul_pt_sum([(E.import_ct(a, lv), p.h) for (a, lv), p in zip(cts, pats)]))
                assert np.array_equal(got, O.rescale(l, pre)), (l, n, ck)
        # the closed form: 8 pairs at one level, everything q - 1
        cts = [(rig.ct(l, "top", 0), l)] * 8
        pats = [rig.mask(l, "top")] * 8
        pre = mul_pt_sum_model(rig, l, cts, pats)
        assert (pre == 8).all(), l
        got = E.export(E.mul_pt_sum([(E.import_ct(a, lv), p.h) for (a, lv), p in zip(cts, pats)]))
        assert not got.any(), l
        with pytest.raises(RuntimeError, match=r"mul_pt_sum: 1\.\.8"):
            E.mul_pt_sum([(E.import_ct(cts[0][0], l), pats[0].h)] * 9)
        one = [(rig.ct(l, "corners", 130), l)]
        got = E.export(E.mul_pt_sum([(E.import_ct(one[0][0], l), rig.mask(l, "small").h)]))  # usable after the refusal
        assert np.array_equal(got, O.rescale(l, mul_pt_sum_model(rig, l, one, [rig.mask(l, "small")]))), l
