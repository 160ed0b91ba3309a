"""The one list of operations that between them take every form of a complete key switch (csrc/engine.hip
run_ks): shared by tests/test_gpu_fused_ki.py (fused against separate launches) and tools/keyswitch_digest.py
(the residues, levels, launches and counters pinned against tests/golden/keyswitch_digests.json).

operations(E, sparse) yields (name, [results]) one operation at a time: an operation runs when the generator is
advanced to it, so a caller can take counters around each.  run(E, sparse) is the flat list of exported bytes."""
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
