"""The key switch at its digit extremes with CHOSEN keys (tests/test_gpu_keyswitch_shapes.py): the parameter sets, the
evaluation-only engine that takes any reduced key (import_ksk), the edge operands -- and, run as a script, the digests
of the raw key-switch core on sets A, C and D as one JSON line.  The fused key-switch core (AESFHE_FUSED_KI) and its
8-residue form (AESFHE_KI8) are read once per process, so the test runs this file in fresh child processes with each
switched off and compares the digests with the default run's."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (str(ROOT), str(ROOT / "aes-implementation-fhe_amd"), str(Path(__file__).resolve().parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

import edge_patterns as ep  # noqa: E402

# set -> (log N, max_level, dnum): alpha = ceil((max_level + 2) / dnum) limbs per digit, alpha + 1 special primes
SETS = {
    "A": (13, 13, 1),    # alpha 15, 16 special primes, 1 digit: ModUp of 15 sources, ModDown of 16
    "B": (13, 17, 2),    # alpha 10, 11 special primes, 2 digits
    "C": (13, 17, 10),   # alpha 2, 3 special primes, 10 digits: one fold of the inner product, run-time digit loop
    "D": (13, 17, 19),   # alpha 1, 2 special primes, 19 digits: two folds, 19 of 24 conversion groups
    "E": (16, 13, 1),    # A on the N = 2^16 kernels
}
KEY_KINDS = ("top", "corners", "uniform")
D_KINDS = ("corners", "top", "conv_top", "uniform")
SEED = 0x5EED


def oracle(name):
    from oracle.ckks_cpu import OracleParams
    log_n, L, dnum = SETS[name]
    return OracleParams(log_n=log_n, max_level=L, dnum=dnum, seed=SEED)


def key_moduli(O):
    """the moduli of a full key's rows: the n_ks chain limbs, then the special primes"""
    return np.concatenate([O.moduli[: O.n_ks], O.moduli[O.n_q:]])


def make_key(O, kind, seed=1):
    """[dnum][2][n_ks + n_p][N], every residue reduced: a key only in shape -- the key switch is linear algebra on
    whatever it is given, and the oracle runs the same array"""
    q = key_moduli(O)
    if kind == "top":
        return np.ascontiguousarray(np.broadcast_to(ep.top(q, O.n), (O.dnum, 2, len(q), O.n)))
    f = ep.corners if kind == "corners" else ep.uniform
    return np.stack([np.stack([f(q, O.n, seed + 2 * j + h) for h in range(2)]) for j in range(O.dnum)])


def make_d(O, level, kind, seed=2):
    nl = O.nl(level)
    q = O.moduli[:nl]
    if kind == "top":
        return ep.top(q, O.n)
    if kind == "conv_top":
        return ep.conv_top_digits(O, nl, O.alpha)
    return (ep.corners if kind == "corners" else ep.uniform)(q, O.n, seed + level)


def levels(O):
    return (O.L, O.L // 2, 0)


def build_engine(name, O, key, tags=(0,)):
    """an evaluation-only engine of the set with `key` imported under every tag of `tags`; eager products (the tensor
    fold of the inner product), no deferred calls, the oracle's full special basis"""
    from mi355x_ckks import Engine
    log_n, L, dnum = SETS[name]
    E = Engine.evaluation_only(prng_key=bytes(range(32)), log_n=log_n, max_level=L, dnum=dnum, allow_insecure=True,
                               enc_nonce=1, lazy=False, defer_calls=False)
    E.set_low_p(False)
    assert np.array_equal(E.moduli(), O.moduli)
    assert (E.alpha, E.n_p, E.n_ks) == (O.alpha, O.n_p, O.n_ks)
    E.import_pk(np.zeros((2, E.n_q, E.n), np.uint32))  # import_ct and the debug calls ask for a public key; none is used
    for g in tags:
        E.import_ksk(g, -1, key)
    return E


def main():
    out = {}
    for name in ("A", "C", "D"):
        O = oracle(name)
        for kind in KEY_KINDS:
            E = build_engine(name, O, make_key(O, kind))
            for level in levels(O):
                for dk in D_KINDS:
                    r = E.debug_keyswitch(level, 0, make_d(O, level, dk))
                    out[f"{name}/{kind}/{level}/{dk}"] = hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest()[:24]
            del E
    print(json.dumps(out))


if __name__ == "__main__":
    main()
