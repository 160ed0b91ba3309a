"""Bit-identity record of the complete key switch (csrc/engine.hip run_ks / run_moddown: ModUp, key inner product,
ModDown) through every entry point that builds one: python3 tools/keyswitch_digest.py [LIB.so] prints, per case and
per operation of tests/helpers/keyswitch_ops.py, a SHA-256 of the exported residues of every result (the members of
a stack one by one), the results' levels, and what the operation added to the process's kernel launches and to
every engine counter (--golden COMMIT: in the form of tests/golden/keyswitch_digests.json, recorded from a build of
that commit).  tests/test_gpu_keyswitch_digest.py compares the result with that file.

--list hoisted: the same record of the second list, hoisted_operations -- the hoisted and accumulating key switches
(Hoist, giant_accumulate_many) -- over HOISTED_CASES, in the form of tests/golden/hoisted_digests.json.

--list products: the third list, product_operations -- the ciphertext x ciphertext products (mul, mul_many, the power
basis, EvalMod) -- over PRODUCT_CASES, in the form of tests/golden/product_digests.json.

An operation is measured together with the export of its results: calls are deferred by default, and an export
settles what a result still owes (a lazy product's relinearisation runs there).

A case is an engine (pinned seed and encryption nonce) under one setting of the switches the engine reads at
construction; the environment is set before the engine is built and restored afterwards.  AESFHE_FUSED_CONV is read
once per process and stays with tests/test_gpu_fused_conv.py."""
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "tests" / "helpers"), str(ROOT), str(ROOT / "aes-implementation-fhe_amd")]

import mi355x_ckks  # noqa: E402
from keyswitch_ops import exported  # noqa: E402


def _boot13():
    """log N 13, bootstrappable, one digit per limb group of 5: the list with the sparse bootstrap (d2s, double primes)"""
    return mi355x_ckks.Engine(log_n=13, use_bootstrap=True, max_level=3, dnum=5, seed=11, allow_insecure=True, enc_nonce=0)


def _deep13():
    """log N 13, 6 levels, 3 digits: levels enough for the fused rescale, more than one digit"""
    return mi355x_ckks.Engine(log_n=13, max_level=6, dnum=3, seed=0xC0DE, allow_insecure=True, enc_nonce=0)


def _ring16():
    """log N 16: the ring k_bx_cols exists for"""
    from engine_context import EngineContext
    return EngineContext(signature=1, max_level=17, log_n=16, seed=0x5EED, enc_nonce=0).engine


def _env(ki="1", rev="1", bx="0"):
    return {"AESFHE_FUSED_KI": ki, "AESFHE_CONJ_REV": rev, "AESFHE_BX_COLS": bx}


# case -> (engine, with the bootstrap, switches)
CASES = {}
for _ki in "01":
    for _rev in "01":
        CASES[f"n13_boot_ki{_ki}_rev{_rev}"] = (_boot13, True, _env(_ki, _rev))
        CASES[f"n13_deep_ki{_ki}_rev{_rev}"] = (_deep13, False, _env(_ki, _rev))
CASES["n16_default"] = (_ring16, False, _env())
CASES["n16_bx_cols"] = (_ring16, False, _env(bx="1"))


# the second list: the default, and each switch that alone reaches a path -- trace4 from the first trace step, the
# single giant_accumulate, the unfused giant_accumulate_many loop, materialised baby steps, the non-double-hoisted ends
HOISTED_SWITCHES = ("AESFHE_S2D_TRACE", "AESFHE_GIANT_BATCH", "AESFHE_FUSED_GIANT", "AESFHE_FUSED_BABY", "AESFHE_DOUBLE_HOIST")


def _henv(off=None):
    return {**_env(), **{k: "0" if k == off else "1" for k in HOISTED_SWITCHES}}


HOISTED_CASES = {"n13_deep": (_deep13, False, _henv()), "n13_boot": (_boot13, True, _henv())}
for _k in HOISTED_SWITCHES:
    HOISTED_CASES["n13_boot_" + _k[len("AESFHE_"):].lower() + "0"] = (_boot13, True, _henv(_k))
# log N 16: the only ring whose plans reach the fused-core form of giant_accumulate_many (a group's sole accumulation)
HOISTED_CASES["n16_boot"] = (_ring16, "only", _henv())
HOISTED_CASES["n16_boot_fused_giant0"] = (_ring16, "only", _henv("AESFHE_FUSED_GIANT"))

# the third list, the products: the default, and each switch of the product path on the engine where it reaches a path of
# its own -- the tensor first, relinearisation and rescale apart, one mul per pair, EvalMod's 2 P - 1 as a lincomb
PRODUCT_SWITCHES = ("AESFHE_FUSED_TENSOR", "AESFHE_FUSED_RESCALE", "AESFHE_BATCH_OPS", "AESFHE_FUSED_AFFINE")


def _penv(off=None):
    return {**_env(), **{k: "0" if k == off else "1" for k in PRODUCT_SWITCHES}}


PRODUCT_CASES = {"n13_deep": (_deep13, False, _penv()), "n13_boot": (_boot13, True, _penv())}
for _k in PRODUCT_SWITCHES[:3]:
    PRODUCT_CASES["n13_deep_" + _k[len("AESFHE_"):].lower() + "0"] = (_deep13, False, _penv(_k))
for _k in ("AESFHE_FUSED_AFFINE", "AESFHE_FUSED_TENSOR"):
    PRODUCT_CASES["n13_boot_" + _k[len("AESFHE_"):].lower() + "0"] = (_boot13, True, _penv(_k))

# list -> (cases, the generator's name in tests/helpers/keyswitch_ops.py: looked up when a list is run, so the tool
# loads beside a helper that has only the first list)
LISTS = {"keyswitch": (CASES, "operations"), "hoisted": (HOISTED_CASES, "hoisted_operations"),
         "products": (PRODUCT_CASES, "product_operations")}


def case_digests(case: str, which: str = "keyswitch") -> dict:
    """{operation: {"sha256", "level", "launches", "counters"}} in the order the operations ran"""
    import keyswitch_ops
    cases, gen = LISTS[which]
    make, sparse, env = cases[case]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        E = make()
        E._ensure_keys()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out = {}
    ops = getattr(keyswitch_ops, gen)(E, sparse)
    while True:
        l0, c0 = mi355x_ckks.launch_count(), E.counters()
        try:
            name, res = next(ops)
        except StopIteration:
            break
        h = hashlib.sha256()
        for b in exported(E, res):
            h.update(b)
        c1 = E.counters()
        out[name] = {"sha256": h.hexdigest(), "level": [x.level for x in res], "launches": mi355x_ckks.launch_count() - l0,
                     "counters": {k: c1[k] - c0[k] for k in c1 if c1[k] != c0[k]}}
    return out


def main():
    """[LIB.so] [--list keyswitch|hoisted|products] [--golden COMMIT] [--cases A,B]: the golden file's form, naming the commit
    the library was built from"""
    args = sys.argv[1:]
    opt = {}
    for flag in ("--list", "--golden", "--cases"):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    which, commit = opt.get("--list", "keyswitch"), opt.get("--golden")
    cases = opt["--cases"].split(",") if "--cases" in opt else list(LISTS[which][0])
    if args:
        mi355x_ckks.load_library(Path(args[0]))
    got = {c: case_digests(c, which) for c in cases}
    print(json.dumps({"parent": commit, "cases": got} if commit else got, indent=1, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
