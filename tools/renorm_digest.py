"""Bit-identity record of the secret-key renorm (csrc/engine.hip RenormSpec / renorm): python3
tools/renorm_digest.py [LIB.so] prints, for every renorm shape, codec and re-encryption path, a digest of
the output ciphertexts' residues, their levels and the kernel launches the call issued (--golden COMMIT:
in the form of tests/golden/renorm_digests.json, recorded from a build of that commit).

digests() -> {case: {"digest": blake2b-16 hex of E.export() of every output in order (the members of a
stacked output one by one), "level": [...], "launches": {kernel id: count}}} -- plus, where a case says so,
the engine's "relin" / "rescale" counters over the call (_inputs) or the growth of the device buffer pool
(_pool: a slab that is not retired shows only there).  The cases run in a fixed
order on engines of their own (GROUPS: one engine per group, so one diverging case shifts only its
group): the encryption counter never resets, so a digest depends on every encryption made before it.
tests/test_gpu_renorm_digest.py compares the result with tests/golden/renorm_digests.json.

Inputs are tiled 256 zeta16^nib with a phase jitter within +-pi/40 (far inside the snap margin: the
snapped message cannot depend on accumulation order)."""
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "aes-implementation-fhe_amd")]

import mi355x_ckks  # noqa: E402

SEED = 0xD16E57  # no test's engine uses it
Z16 = np.exp(-2j * np.pi / 16)
# ShiftRows on the column-major state (byte i = 4 col + row): output byte i <- input byte SR[i]
SR = [4 * ((i // 4 + i % 4) % 4) + i % 4 for i in range(16)]


def _engine(env=None):
    """the recorder's own engine; env: flags the engine reads at construction, restored afterwards"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        E = mi355x_ckks.Engine(log_n=13, max_level=6, dnum=3, seed=SEED, allow_insecure=True, enc_nonce=SEED)
        E._ensure_keys()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return E


def _msg(E, period, seed):
    rng = np.random.default_rng(seed)
    nib = rng.integers(0, 16, period)
    z = 256.0 * Z16 ** nib * np.exp(1j * rng.uniform(-np.pi / 40, np.pi / 40, period))
    return np.tile(z, E.slot_count // period)


def _noisy(E, period, seed):
    return E.encrypt(_msg(E, period, seed))


def _split(E, period, seed):
    """(a, b) with a + conj(b) = the noisy message: a conjugate-split pair (S1, S2)"""
    z = _msg(E, period, seed)
    rng = np.random.default_rng(seed + 1000)
    d = np.tile(rng.normal(size=period) + 1j * rng.normal(size=period), E.slot_count // period)
    return E.encrypt(0.5 * z + d), E.encrypt(np.conj(0.5 * z - d))


def _case(E, out, name, fn, **extra):
    """run fn() (the renorm call alone: its inputs exist already) and record its outputs"""
    before = mi355x_ckks.alg_bytes()
    res = fn()
    after = mi355x_ckks.alg_bytes()
    res = list(res) if isinstance(res, (tuple, list)) else [res]
    h = hashlib.blake2b(digest_size=16)
    for c in res:
        for m in (E.unstack(c) if E.members(c) > 1 else [c]):
            h.update(E.export(m).tobytes())
    launches = {k: after[k][1] - before[k][1] for k in after if after[k][1] != before[k][1]}
    out[name] = {"digest": h.hexdigest(), "level": [c.level for c in res], "launches": launches, **extra}


def _pair(E, out):
    S = E.slot_count
    _case(E, out, "pair_states1", lambda a=_noisy(E, S, 1), b=_noisy(E, S, 2): E.renorm_pair(a, b))
    _case(E, out, "pair_states3", lambda a=_noisy(E, S, 3), b=_noisy(E, S, 4): E.renorm_pair(a, b, 3))
    _case(E, out, "pair_states3_level4", lambda a=_noisy(E, S, 5), b=_noisy(E, S, 6): E.renorm_pair(a, b, 3, 4))


def _periodic(E, out):
    h, l = _noisy(E, 16, 10), _noisy(E, 16, 11)
    _case(E, out, "periodic16", lambda: E.renorm_periodic(h, l, 16))
    _case(E, out, "periodic16_level3", lambda: E.renorm_periodic(h, l, 16, 3))
    (h1, h2), (l1, l2) = _split(E, 16, 12), _split(E, 16, 13)
    _case(E, out, "periodic16_conj", lambda: E.renorm_periodic(h1, l1, 16, None, conj=(h2, l2)))
    low = E.level_down(l2, E.max_level - 2)  # a partner at another level: summed homomorphically first
    _case(E, out, "periodic16_conj_dropped", lambda: E.renorm_periodic(h1, l1, 16, None, conj=(h2, low)))
    h64, l64 = _noisy(E, 64, 14), _noisy(E, 64, 15)
    _case(E, out, "periodic64", lambda: E.renorm_periodic(h64, l64, 64))


def _perm_pack(E, out):
    h, l = _noisy(E, 16, 20), _noisy(E, 16, 21)
    (h1, h2), (l1, l2) = _split(E, 16, 22), _split(E, 16, 23)
    for pack in (False, True):
        tag = "perm_pack" if pack else "perm"
        _case(E, out, tag, lambda: E.renorm_periodic_perm(h, l, 16, SR, None, pack=pack))
        _case(E, out, tag + "_conj", lambda: E.renorm_periodic_perm(h1, l1, 16, SR, None, conj=(h2, l2), pack=pack))
    _case(E, out, "pack", lambda: E.renorm_pack(h, l, 16))
    _case(E, out, "pack_conj", lambda: E.renorm_pack(h1, l1, 16, None, conj=(h2, l2)))


def _single(E, out):
    x = _noisy(E, E.slot_count, 30)
    _case(E, out, "single", lambda: E.renorm_single(x))
    x32 = _noisy(E, 32, 31)
    _case(E, out, "single32", lambda: E.renorm_single(x32, None, period=32))
    a, b = _split(E, 32, 32)
    _case(E, out, "single32_conj", lambda: E.renorm_single(a, None, period=32, conj=b))
    x64 = _noisy(E, 64, 33)
    _case(E, out, "single64", lambda: E.renorm_single(x64, None, period=64))


def _unpack(E, out):
    x = _noisy(E, 32, 40)
    a, b = _split(E, 32, 41)
    _case(E, out, "unpack16", lambda: E.renorm_unpack(x, 16))
    _case(E, out, "unpack16_conj", lambda: E.renorm_unpack(a, 16, None, conj=b))
    _case(E, out, "unpack16_perm", lambda: E.renorm_unpack_perm(x, 16, SR))
    _case(E, out, "unpack16_perm_conj", lambda: E.renorm_unpack_perm(a, 16, SR, None, conj=b))
    x64 = _noisy(E, 64, 42)
    _case(E, out, "unpack32", lambda: E.renorm_unpack(x64, 32))


def _inputs(E, out):
    """inputs that are not plain two-polynomial ciphertexts; each records what the renorm did with it:
    "relin" / "rescale": the engine's counters over the call (an unrelinearised product is decrypted with
    s^2, so no relinearisation; owed rescales are decrypted at the raw scale while the CRT limbs cover it)"""
    one = E.encrypt(np.ones(E.slot_count))
    l = _noisy(E, 16, 51)

    def counted(name, h):
        c0 = E.counters()
        _case(E, out, name, lambda: E.renorm_periodic(h, l, 16))
        c1 = E.counters()
        out[name].update({k: c1[k] - c0[k] for k in ("relin", "rescale")})

    counted("input_plain", _noisy(E, 16, 53))  # fills the pool: the next two show their own work only
    prod = E._raw_mul(_noisy(E, 16, 50), one, relin=False)
    assert prod.num_polys == 3
    counted("input_3poly", prod)
    owed = E._raw_mul(E._raw_mul(_noisy(E, 16, 52), 0.5), 0.5)  # two owed rescales (the most the API leaves)
    counted("input_owed_rescales", owed)


def _stacks(E, out):
    S = E.slot_count

    def stk(period, seed):
        return E.stack([_noisy(E, period, seed + k) for k in range(3)])

    _case(E, out, "stack3_pair", lambda a=stk(S, 60), b=stk(S, 63): E.renorm_pair(a, b))
    _case(E, out, "stack3_periodic16", lambda a=stk(16, 66), b=stk(16, 69): E.renorm_periodic(a, b, 16))
    _case(E, out, "stack3_unpack16", lambda a=stk(32, 72): E.renorm_unpack(a, 16))
    _case(E, out, "stack3_single", lambda a=stk(S, 75): E.renorm_single(a))


def _pool(E, out):
    x = _noisy(E, 32, 80)
    E.renorm_pool(2)
    for k in range(5):  # the third and the fifth draw from a refilled pool and retire the slab before
        b0 = E.pool_stats()["bytes"]
        _case(E, out, f"pool2_single32_{k}", lambda: E.renorm_single(x, None, period=32))
        if k >= 3:  # steady state: a refill reuses the retired slab, the device pool does not grow
            out[f"pool2_single32_{k}"]["pool_growth"] = E.pool_stats()["bytes"] - b0
    E.renorm_pool(0)
    h, l = _noisy(E, 16, 81), _noisy(E, 16, 82)
    _case(E, out, "nopool_periodic16", lambda: E.renorm_periodic(h, l, 16))
    _case(E, out, "nopool_single32", lambda: E.renorm_single(x, None, period=32))
    _case(E, out, "nopool_unpack16", lambda: E.renorm_unpack(x, 16))
    _case(E, out, "nopool_pack", lambda: E.renorm_pack(h, l, 16))


def _flagged(tag):
    def run(E, out):
        h, l, x = _noisy(E, 16, 90), _noisy(E, 16, 91), _noisy(E, 32, 92)
        _case(E, out, tag + "_periodic16", lambda: E.renorm_periodic(h, l, 16))
        _case(E, out, tag + "_single32", lambda: E.renorm_single(x, None, period=32))
        _case(E, out, tag + "_unpack16", lambda: E.renorm_unpack(x, 16))
    return run


# group -> (flags read at engine construction, the group's cases)
GROUPS = {
    "pair": (None, _pair), "periodic": (None, _periodic), "perm_pack": (None, _perm_pack), "single": (None, _single),
    "unpack": (None, _unpack), "inputs": (None, _inputs), "stacks": (None, _stacks), "pool": (None, _pool),
    "sparse_dec_off": ({"AESFHE_SPARSE_DEC": "0"}, _flagged("sparse_dec_off")),
    "snap_encode_off": ({"AESFHE_SNAP_ENCODE": "0"}, _flagged("snap_encode_off")),
    "direct32_off": ({"AESFHE_RENORM_DIRECT32": "0"}, _flagged("direct32_off")),
}


def group_digests(group: str) -> dict:
    env, cases = GROUPS[group]
    out = {}
    cases(_engine(env), out)
    return out


def digests() -> dict:
    out = {}
    for g in GROUPS:
        out.update(group_digests(g))
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
