"""The one list of operations that between them take every form of a complete key switch (csrc/engine.hip
run_ks): shared by tests/test_gpu_fused_ki.py (fused against separate launches) and tools/keyswitch_digest.py
(the residues, levels, launches and counters pinned against tests/golden/keyswitch_digests.json).

operations(E, sparse) yields (name, [results]) one operation at a time: an operation runs when the generator is
advanced to it, so a caller can take counters around each.  run(E, sparse) is the flat list of exported bytes.

hoisted_operations(E, boot) is the second list, of the same form: the hoisted and accumulating key switches (one
ModUp for several inner products, sums across calls; csrc/engine.hip Hoist, giant_accumulate_many), pinned against
tests/golden/hoisted_digests.json.  It is a list of its own so that the first list's encryptions, and so its
digests, stay where they are.

product_operations(E, boot) is the third, again with an rng of its own: the ciphertext x ciphertext products (csrc/engine.hip
mul, mul_many, and through them the power basis and EvalMod), pinned against tests/golden/product_digests.json."""
import numpy as np


def operations(E, sparse: bool):
    rng = np.random.default_rng(23)
    zs = [np.exp(2j * np.pi * rng.random(E.slot_count)) for _ in range(6)]
    a, b, c = (E.encrypt(z) for z in zs[:3])
    prod = E.multiply(a, b, "rlk")                                       # lazy product (deferred relinearisation)
    yield "relinearize", [E.relinearize(E.multiply(a, b))]               # keyswitch (relin_raw)
    yield "relin_rescale", [E.add(prod, c)]                              # normalize: relin fused with its rescale
    yield "multiply_many3", E.multiply_many([(a, b), (b, c), (a, c)])    # tensor fold, 3 members
    yield "multiply_many_squared", E.multiply_many([(a, a), (b, c)])     # a squared pair: both factors one buffer
    yield "rotate", [E.rotate(a, None, 3)]                               # permuted copy + keyswitch
    yield "conjugate", [E.conjugate(a)]                                  # reversed own digit
    yield "conjugate_lazy_tensor", [E.conjugate(prod)]                   # deferred tensor: two summed sources
    yield "conjugate_many", E.conjugate_many([b, E.multiply(c, 0.5 + 0.25j)])  # canonical + deferred 2-polynomial
    st = E.stack([E.encrypt(z) for z in zs[:4] + zs[:4] + zs[:2]])       # 10 members: chunked key switches
    yield "stack10_multiply", [E.multiply(st, st, "rlk")]
    yield "stack10_conjugate", [E.conjugate(st)]
    yield "stack10_rotate", [E.rotate(st, None, 3)]                      # chunked plain keyswitch with addends
    if sparse:
        P = 32
        z = np.exp(2j * np.pi * rng.random(P))
        yield "bootstrap_sparse32", [E.bootstrap_sparse(E.encrypt(np.tile(z, E.slot_count // P)), P)]


def hoisted_operations(E, boot):
    """boot: False (no bootstrap), True, or "only" (the full-slot and the sparse bootstrap alone: the log N 16 cases)"""
    rng = np.random.default_rng(29)
    sc = E.slot_count
    zs = [np.exp(2j * np.pi * rng.random(sc)) for _ in range(6)]
    if boot == "only":
        yield "bootstrap", [E.bootstrap(E.encrypt(0.5 * zs[0]))]
        yield "bootstrap_sparse32", [E.bootstrap_sparse(E.encrypt(np.tile(zs[1][:32], sc // 32)), 32)]
        return
    a, b, f0, f1, f2 = (E.encrypt(z) for z in zs[:5])
    yield "rotate_hoisted", E.rotate_many(a, [1, 0, -3, 1])              # a zero step and a repeat
    rot, conj = E.galois_rotate, E.galois_conj
    p0, p1 = E._raw_mul(a, 0.5 + 0.25j), E._raw_mul(b, 0.25 - 0.5j)      # deferred scalar products: stacked rescale,
    low = E.level_down(E.encrypt(zs[5]), a.level - 2)                    # sources at a regular stride; a second chunk
    yield "galois_multi", E.galois_multi([
        (a, rot(1)), (a, rot(-5)), (a, conj), (b, conj), (a, 1),         # one source three times, a second, identity
        (p0, rot(2)), (p1, rot(7)), (low, rot(3)),
        (f2, rot(4)), (f0, conj), (f1, rot(-2))])                        # unrelated sources, out of order: gathered c1
    own = [(np.arange(sc) % 3 == i).astype(np.complex128) for i in range(3)]
    m = [E.encode(v) for v in own]
    yield "rot_pt_sum1", E.rot_pt_sum(a, [0, 3, -5], [m])
    yield "rot_pt_sum2", E.rot_pt_sum(b, [0, 3, -5], [[m[0], m[1], m[2]], [m[1], None, None]])  # the second: unrotated only
    fill = E.encode(np.exp(2j * np.pi * rng.integers(0, 16, sc) / 16))
    yield "rot_pt_affine", E.rot_pt_affine(a, [0, 16, -7], [[m[2], m[0], m[1]]], [fill])
    if boot:
        P = 32
        tiled = [np.tile(np.exp(2j * np.pi * rng.random(P)), sc // P) for _ in range(3)]
        yield "bootstrap", [E.bootstrap(E.encrypt(0.5 * zs[0]))]
        yield "bootstrap_sparse32", [E.bootstrap_sparse(E.encrypt(tiled[0]), P)]       # trace steps: s2d_trace4, trace4
        yield "bootstrap_pair_sparse32", list(E.bootstrap_pair_sparse(E.encrypt(tiled[1]), E.encrypt(tiled[2]), P))  # nb = 2


def product_operations(E, boot):
    """the ciphertext x ciphertext products (csrc/engine.hip mul, mul_many and what drives them): the undeferred calls,
    so that each operation is the engine call it names.  boot: the engine has the bootstrap (EvalMod's 2 P - 1 flags)"""
    rng = np.random.default_rng(31)
    sc = E.slot_count
    zs = [np.exp(2j * np.pi * rng.random(sc)) for _ in range(6)]
    a, b, c, d, e = (E.encrypt(z) for z in zs[:5])
    low = E.level_down(E.encrypt(zs[5]), a.level - 2)
    p = E._raw_mul(a, 0.5 + 0.25j)                                       # a deferred scalar product: owes a rescale
    st3, st10 = E.stack([a, b, c]), E.stack([a, b, c, d, e, a, c, e, b, d])
    E.set_lazy(False)
    yield "mul", [E._raw_mul(a, b)]
    yield "mul_squared", [E._raw_mul(a, a)]
    yield "mul_level_down", [E._raw_mul(a, low)]
    yield "mul_pending", [E._raw_mul(a, p)]
    yield "mul_stack3", [E._raw_mul(st3, st3)]                           # one key-switch chunk where the level allows
    yield "mul_stack10", [E._raw_mul(st10, st10)]                        # more than a chunk: the tensor first
    yield "mul_tensor", [E._raw_mul(a, b, relin=False)]                  # three polynomials
    E.set_lazy(True)
    yield "mul_lazy_add", [E._raw_add(E._raw_mul(a, b), c)]              # the add settles the product (normalize)
    yield "many1", E.multiply_many([(a, b)])
    yield "many3", E.multiply_many([(a, b), (b, c), (c, d)])
    yield "many10", E.multiply_many([(a, b), (a, c), (a, d), (a, e), (b, c), (b, d), (b, e), (c, d), (c, e), (d, e)])
    yield "many_two_levels", E.multiply_many([(a, b), (low, c), (d, e)])
    yield "many_level_down", E.multiply_many([(low, a), (low, b), (c, low)])  # three drops to one level: convert_many
    yield "many_squared", E.multiply_many([(a, a), (b, c)])
    yield "many_with_stack", E.multiply_many([(st3, st3), (a, b)])       # a stacked operand: one mul per pair
    yield "power_basis5", E.make_power_basis(a, 5)
    if boot:
        yield "bootstrap", [E.bootstrap(E.encrypt(0.5 * zs[0]))]
        yield "bootstrap_sparse32", [E.bootstrap_sparse(E.encrypt(np.tile(zs[1][:32], sc // 32)), 32)]
        limbs = E.level_limbs
        double = [l for l in range(1, len(limbs)) if limbs[l] - limbs[l - 1] == 2]
        if double:  # the first double-prime level: a product of operands there is formed one level below
            lv = double[0]                   # (nothing encrypts that high: uniform residues imported there)
            q = E.moduli()[:E.nl(lv)]
            x = E.import_ct(np.array([[rng.integers(0, int(m), E.n) for m in q] for _ in range(2)], np.uint32), lv)
            E.set_lazy(False)
            yield "mul_squared_boundary", [E._raw_mul(x, x)]


def exported(E, results):
    """the residues of every result, the members of a stack one by one"""
    flat = []
    for x in results:
        flat += E.unstack(x) if E.members(x) > 1 else [x]
    return [E.export(x).tobytes() for x in flat]


def run(E, sparse: bool):
    out = []
    for _, res in list(operations(E, sparse)):  # every operation first, then the exports (which settle what is owed)
        out += res
    return exported(E, out)
