"""Bit-identity record of the three public-operand multiply-accumulate ops (csrc/engine.hip: lut_eval_public,
xor_value_public, xor_value_typed) and their debug readbacks: python3 tools/public_mac_digest.py [LIB.so]
prints, per case, renorm_digest's record (a digest of the exported output residues, the output levels, the kernel
launches of the call) plus the engine's "rescale" counter over the call alone (--golden COMMIT: in the form of
tests/golden/public_mac_digests.json, recorded from a build of that commit).
tests/test_gpu_public_mac_digest.py compares the result with that file.

Every group runs on an engine of its own (renorm_digest._engine: log N 13, 6 levels).  Operands are import_ct of
seeded uniform residues, so no encryption is involved; the one operand that owes a rescale is a deferred scalar
product of such a ciphertext.  The debug rows are digested as raw bytes."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "tools"), str(ROOT), str(ROOT / "aes-implementation-fhe_amd")]

import mi355x_ckks  # noqa: E402
from renorm_digest import _case, _engine  # noqa: E402

LUT_ROWS = (1, 3, 5, 7)  # the rows of the XOR4's c1 / c2 tables that hold a coefficient
HEAVY = 2.0 ** 24        # |weight| of the typed case whose raw scale has no headroom: rescaled inside the call


def ct(E, level, rng):
    """a two-polynomial ciphertext of uniform residues at `level`"""
    q = E.moduli()[:E.nl(level)]
    return E.import_ct(np.stack([np.stack([rng.integers(0, int(m), E.n, dtype=np.uint64) for m in q]) for _ in range(2)]).astype(np.uint32),
                       level)


def nibbles(E, rng, k=1):
    return [rng.integers(0, 16, E.slot_count).astype(np.uint8) for _ in range(k)]


def value_tables(gain):
    from coeffgen import xor_value_table
    tab = xor_value_table()[:9]
    return np.ascontiguousarray(16.0 * gain * tab), np.ascontiguousarray(gain * tab)


def mixed_powers(E, rng, top):
    """hi^p / lo^p stand-ins for p = 1..8: two one level lower, one owing a rescale (common level top - 1)"""
    a_hi = {p: ct(E, top, rng) for p in range(1, 9)}
    a_lo = {p: ct(E, top, rng) for p in range(1, 9)}
    a_hi[3], a_lo[8] = ct(E, top - 1, rng), ct(E, top - 1, rng)
    a_lo[5] = E.multiply(ct(E, top, rng), 0.625)
    return a_hi, a_lo


def flat_powers(E, rng, level):
    return {p: ct(E, level, rng) for p in range(1, 9)}, {p: ct(E, level, rng) for p in range(1, 9)}


def _counted(E, out, name, fn):
    """_case plus the rescales of fn() alone (the export behind the digest settles what the outputs still owe)"""
    box = {}

    def run():
        c0 = E.counters()["rescale"]
        res = fn()
        box["rescale"] = E.counters()["rescale"] - c0
        return [c for pr in res for c in pr] if isinstance(res, list) else [c for c in res if c is not None]

    _case(E, out, name, run)
    out[name].update(box)


def _value(E, out):
    rng = np.random.default_rng(0xA1)
    for name, gain in (("value_mixed_gain256", 1.0 / 256.0), ("value_mixed_gain3", 1.0 / 3.0)):
        a_hi, a_lo = mixed_powers(E, rng, 6)
        nib = nibbles(E, rng, 2)
        _counted(E, out, name, lambda: E.xor_value_public(a_hi, a_lo, *nib, *value_tables(gain)))
    a_hi, a_lo = flat_powers(E, rng, 2)
    nib = nibbles(E, rng, 2)
    _counted(E, out, "value_level2", lambda: E.xor_value_public(a_hi, a_lo, *nib, *value_tables(1.0 / 256.0)))


def typed_weights(E, rng, groups):
    """weights in [-1/128, 1/128] with a third of the slots at 0, flags on a quarter of the slots"""
    sc = E.slot_count
    w = rng.uniform(-1.0 / 128.0, 1.0 / 128.0, (groups, sc))
    w[rng.random((groups, sc)) < 1.0 / 3.0] = 0.0
    return np.ascontiguousarray(w), np.ascontiguousarray((rng.random((groups, sc)) < 0.25).astype(np.uint8))


def _typed(E, out):
    rng = np.random.default_rng(0xA2)
    for groups in (1, 2):
        a_hi, a_lo = mixed_powers(E, rng, 6)
        nib = nibbles(E, rng, 2)
        w, f = typed_weights(E, rng, groups)
        _counted(E, out, f"typed_groups{groups}", lambda: E.xor_value_typed(a_hi, a_lo, *nib, w, f))
    # level 1 leaves log2 Q_0 - log2 delta_0 - 21 ~ 9 bits for the magnitude; 2^24 x the unit tables' 121 / 8.5 has ~ 31 / 27
    a_hi, a_lo = flat_powers(E, rng, 1)
    nib = nibbles(E, rng, 2)
    w = HEAVY * rng.choice([-1.0, 1.0], E.slot_count)
    _counted(E, out, "typed_heavy_rescaled", lambda: E.xor_value_typed(a_hi, a_lo, *nib, w, None))


def xor4_luts(E):
    from add_round_key import default_xor4_coeffs
    from xor4_lut import public_tables
    tables = public_tables(default_xor4_coeffs())
    return E.lut_create(tables.c1), E.lut_create(tables.c2)


def _lut(E, out):
    rng = np.random.default_rng(0xA3)
    l1, l2 = xor4_luts(E)
    flat = {p: ct(E, 4, rng) for p in LUT_ROWS}
    nib, = nibbles(E, rng)
    _counted(E, out, "lut_one", lambda: E.lut_eval_public(l1, None, flat, nib))
    _counted(E, out, "lut_two", lambda: E.lut_eval_public(l1, l2, flat, nib))
    mixed = {1: ct(E, 6, rng), 3: ct(E, 5, rng), 5: E.multiply(ct(E, 6, rng), 0.625), 7: ct(E, 6, rng)}
    _counted(E, out, "lut_two_mixed", lambda: E.lut_eval_public(l1, l2, mixed, nib))


def _debug(E, out):
    rng = np.random.default_rng(0xA4)
    nib = nibbles(E, rng, 2)
    w, f = typed_weights(E, rng, 2)
    l1, _ = xor4_luts(E)
    for name, fn in (("debug_value_pt", lambda: E.debug_xor_value_pt(*nib, *value_tables(1.0 / 256.0), 3)),
                     ("debug_value_typed_pt", lambda: E.debug_xor_value_typed_pt(*nib, w, f, 3)),
                     ("debug_public_pt", lambda: E.debug_public_pt(l1, nib[0], 3))):
        before = mi355x_ckks.alg_bytes()
        rows, scale = fn()
        after = mi355x_ckks.alg_bytes()
        out[name] = {"digest": hashlib.blake2b(rows.tobytes(), digest_size=16).hexdigest(), "shape": list(rows.shape), "scale": scale,
                     "launches": {k: after[k][1] - before[k][1] for k in after if after[k][1] != before[k][1]}}


GROUPS = {"value": _value, "typed": _typed, "lut": _lut, "debug": _debug}


def group_digests(group: str) -> dict:
    out = {}
    GROUPS[group](_engine(), out)
    return out


def main():
    """[LIB.so] [--golden COMMIT]: the golden file's form, naming the commit the library was built from"""
    args = sys.argv[1:]
    commit = None
    if "--golden" in args:
        i = args.index("--golden")
        commit = args[i + 1]
        del args[i:i + 2]
    if args:
        mi355x_ckks.load_library(Path(args[0]))
    groups = {g: group_digests(g) for g in GROUPS}
    print(json.dumps({"parent": commit, "groups": groups} if commit else groups, indent=1, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
