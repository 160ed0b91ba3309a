"""Result packs on the device (aesfhe_pack_periodic / k_pack_periodic, result_pack.py): G periodic results
as ONE level-0 ciphertext z = sum_j X^(j k') ct_j, k' = N / (2 period G), split by the client in the clear.

* the convention, word for word against aesfhe_debug_mono_pack: T = 2, and T = 4 as [a, c, b, d]; members at one level
  (the batched drop), at mixed levels, one owing a rescale;
* exactness: the pack decrypts to pack_slots of the members' own level-0 decryptions to 1e-9 (the pack's phase IS the sum
  of the members' phases times monomials; 1e-9 covers the float64 embeddings of values <= 32);
* error: a member unpacked differs from its message by at most sum_i e_i + 1e-9, e_i the largest slot error of member i
  dropped to level 0 and decrypted alone (triangle inequality through a projection of norm 1; nothing measured enters);
* end to end at log N 15 (the smallest set of the value-decode pipeline tests), through an evaluation-only server at
  log N 13, and the refusals.

Sets: RAW and BOOT of tests/test_gpu_seeded_ct.py at N = 2^13.  The measured figures are in DESIGN.md §3.28.
"""
import ctypes
import gc

import numpy as np
import pytest

from conftest import gpu_context
from test_gpu_seeded_ct import SETS, _context, _server

pytestmark = pytest.mark.gpu

PERIODS = (16, 64)
COUNTS = (1, 3, 5, 8, 32)


@pytest.fixture(scope="module", params=list(SETS))
def client(request):
    return request.param, _context(request.param)


def _periodic(E, rng, period):
    m = rng.uniform(-1, 1, period) + 1j * rng.uniform(-1, 1, period)
    m /= np.maximum(1.0, np.abs(m))           # |m| <= 1
    return np.tile(m, E.slot_count // period)


@pytest.fixture(scope="module")
def members(client):
    """{period: (messages, ciphertexts)}: 32 random period-periodic messages, |m| <= 1, encrypted once per set; their
    levels cycle through the fresh level (runs of more than eight: the batched drop, twice), 1 and 0"""
    which, C = client
    E = C.engine
    out = {}
    for period in PERIODS:
        rng = np.random.default_rng(1000 + period)
        msgs = [_periodic(E, rng, period) for _ in range(max(COUNTS))]
        cts = []
        for j, m in enumerate(msgs):
            c = C.encrypt(m)
            if j % 8 == 5:
                c = E.level_down(c, 1)
            elif j % 8 == 7:
                c = E.level_down(c, 0)
            cts.append(c)
        out[period] = (msgs, cts)
    return out


@pytest.fixture(scope="module")
def alone(client, members):
    """{period: (level-0 decryptions, e_i)} of the 32 members, each dropped to level 0 and decrypted alone: computed once"""
    which, C = client
    E = C.engine
    out = {}
    for period, (msgs, cts) in members.items():
        dec = [E.decrypt(c if c.level == 0 else E.level_down(c, 0)) for c in cts]
        out[period] = (dec, [float(np.abs(d - m).max()) for d, m in zip(dec, msgs)])
    return out


# ---------------------------------------------------------------- 1. the convention
def test_convention_against_mono_pack(client, members):
    which, C = client
    E = C.engine
    period = 16
    msgs, cts = members[period]
    a, b, c, d = cts[0], cts[1], cts[2], cts[3]            # all at the fresh level: one batched drop
    low = cts[5]                                           # level 1
    assert a.level == E.fresh_level and low.level == 1 and cts[7].level == 0

    def owed():
        r = E._raw_mul(cts[4], 0.625)                      # a deferred scalar product: it owes a rescale
        return r

    def same(x, y):
        assert x.level == y.level == 0 and x.num_polys == y.num_polys == 2
        assert np.array_equal(E.export(x), E.export(y))

    z = E.pack_periodic([a, b], period)
    assert z.level == 0 and z.pack == (2, period)
    same(z, E.debug_mono_pack(a, b, period))
    same(E.pack_periodic([a, low], period), E.debug_mono_pack(a, low, period))            # mixed levels
    same(E.pack_periodic([cts[7], owed()], period), E.debug_mono_pack(cts[7], owed(), period))   # level 0, and an owed rescale
    same(C.pack_periodic([owed(), low], period), E.debug_mono_pack(owed(), low, period))
    # T = 4: pack([a, c, b, d]) = mono_pack(mono_pack(a, b, P), mono_pack(c, d, P), 2 P)
    for quad in ([a, b, c, d], [a, low, owed(), cts[7]], [low, cts[7], b, owed()]):
        x, y, u, v = quad
        want = E.debug_mono_pack(E.debug_mono_pack(x, y, period), E.debug_mono_pack(u, v, period), 2 * period)
        got = E.pack_periodic([x, u, y, v], period)
        assert got.pack == (4, period)
        same(got, want)
    # an absent member is an encryption of zero: T = 3 with the last missing is T = 4 with member 3 absent
    same(E.pack_periodic([a, c, b], period), E.pack_periodic([a, c, b, None], period))
    assert E.check(z) is None                              # every residue below its modulus: exportable


# ---------------------------------------------------------------- 2. exactness and 3. error
@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("count", COUNTS)
def test_pack_is_the_exact_sum_and_members_come_back(client, members, alone, count, period):
    from result_pack import group_size, pack_slots, split_slots
    which, C = client
    E = C.engine
    msgs, cts = members[period]
    dec, errs = alone[period]
    G = group_size(count)
    z = E.pack_periodic(cts[:count], period)
    assert z.level == 0 and z.pack == (G, period) and z.num_polys == 2
    got = E.decrypt(z)
    model = pack_slots(dec[:count], period, E.slot_count)
    exact = float(np.abs(got - model).max())
    print(f"{which} T = {count} (G = {G}) period {period}: |decrypt(pack) - pack_slots(level-0 decryptions)| = {exact:.3g} (bound 1e-9)")
    assert exact < 1e-9
    back = split_slots(got, G, period)
    total = sum(errs[:count])
    worst = max(float(np.abs(back[j] - msgs[j]).max()) for j in range(count))
    one = max(errs[:count])
    print(f"{which} T = {count} (G = {G}) period {period}: worst unpacked member error {worst:.3g}; sum of the members' own e_i {total:.3g} "
          f"(ratio {worst / total:.3g}), largest single e_i {one:.3g} (ratio {worst / one:.3g}, sqrt G = {G ** 0.5:.3g})")
    for j in range(count):
        assert np.abs(back[j] - msgs[j]).max() <= total + 1e-9, j
    for j in range(count, G):
        assert np.abs(back[j]).max() <= total + 1e-9, j     # the empty places of the group hold nothing


# ---------------------------------------------------------------- 4. end to end
def test_end_to_end_values_bank_and_pair(coeff_dir):
    """log N 15, 16 states, periodic (the set of tests/test_gpu_byte_lut.py's pipelines): an encoded pair, no AES rounds;
    to_values, to_lut_bank with three selectors and the pair itself travel as ONE [2][nl(0)][N] array"""
    from aes_keyschedule import load_all_coeffs
    from pipeline import AESPipeline
    from result_pack import dump_results, unpack_results
    from state_encoder import dump_ct
    ctx = gpu_context(log_n=15)
    E = ctx.engine
    pipe = AESPipeline(ctx, load_all_coeffs(coeff_dir), use_hard_renorm_between_steps=True, states=16, periodic=True)
    enc = pipe.encoder
    m = np.random.default_rng(174).permutation(256).astype(np.uint8).reshape(16, 16)
    hi, lo = enc.encode(m)
    X = np.arange(256)
    tables = np.stack([((X >> k) & 1).astype(np.float64) for k in (0, 3, 5, 7)])   # four flag bits of the byte
    select = [np.full((16, 16), 0), np.arange(16) % 3, np.broadcast_to(np.arange(16).reshape(16, 1) % 4, (16, 16))]
    val = pipe.to_values(hi, lo)
    bank = pipe.to_lut_bank(hi, lo, tables, select)
    assert len(bank) == 3
    cts = [val] + list(bank) + [hi, lo]
    E.settle(*cts)
    array, meta = dump_results(ctx, cts)
    assert array.dtype == np.uint32 and array.shape == (2, E.nl(0), E.n) and array.nbytes == 2 * E.nl(0) * E.n * 4
    single = sum(dump_ct(ctx, c)[0].nbytes for c in cts)
    print(f"log N 15: the pack is {array.nbytes / 2 ** 20:.2f} MiB, the {len(cts)} members' dump_ct arrays {single / 2 ** 20:.2f} MiB "
          f"(levels {[c.level for c in cts]})")
    assert single > array.nbytes
    assert (meta["members"], meta["G"], meta["period"]) == (6, 8, 256)
    out = enc.decode_packed(array, meta)
    assert len(out) == 5
    assert np.array_equal(out[4], m)                                        # the pair's bytes, exact
    assert np.array_equal(np.rint(256.0 * out[0]).astype(np.int64), m.astype(np.int64))   # the 8-bit values, exact after rounding
    # the members' messages (float64 models, all periodic) and their own level-0 errors
    models = [enc._float_slots(m / 256.0)] + [enc._float_slots(tables[np.broadcast_to(s, (16, 16)), m]) for s in select]
    st = enc._as_batch(m)
    models += [enc._pack(st >> 4), enc._pack(st & 0x0F)]
    errs = [float(np.abs(E.decrypt(E.level_down(c, 0)) - mod).max()) for c, mod in zip(cts, models)]
    bound = sum(errs) + 1e-9
    slots = unpack_results(ctx, array, meta)
    for j, (s, mod) in enumerate(zip(slots, models)):
        assert np.abs(s - mod).max() <= bound, j
    worst = 0.0
    for j in range(4):
        want = enc.decode_values(cts[j])                                    # the unpacked result, at its own level
        assert out[j].shape == want.shape
        worst = max(worst, float(np.abs(out[j] - want).max()))
        assert np.abs(out[j] - want).max() <= bound, j
    print(f"log N 15: members' own level-0 errors {[f'{e:.3g}' for e in errs]}, sum {sum(errs):.3g}; packed floats differ from the "
          f"unpacked decode_values by at most {worst:.3g}")
    for k in range(3):
        assert np.array_equal(np.rint(out[1 + k]).astype(np.int64), tables[np.broadcast_to(select[k], (16, 16)), m].astype(np.int64))


# ---------------------------------------------------------------- 5. an evaluation-only server
def test_evaluation_only_server_packs_without_keys(client):
    from result_pack import dump_results, pack_results
    from state_encoder import StateEncoder, dump_ct, load_ct
    which, C = client
    E = C.engine
    enc = StateEncoder(C, 4, periodic=True)
    state = np.random.default_rng(31).integers(0, 256, (4, 16)).astype(np.uint8)
    hi, lo = enc.encode(state)
    E.export(E.rotate(hi, delta=1))                        # a key for the bundle
    S = _server(C)
    V = S.engine
    assert S.secret_key is None and not V.has_secret
    shi, slo = [load_ct(S, *dump_ct(C, c)) for c in (hi, lo)]
    assert enc.layout.same(shi.layout)
    slow = V.level_down(slo, 1)                            # a server-side result at another level
    slow.layout = slo.layout
    keys = V.key_ids()
    z = pack_results(S, [shi, slow])
    assert z.level == 0 and z.pack == (2, 64)
    array, meta = dump_results(S, [shi, slow])
    assert V.key_ids() == keys                             # aesfhe_eval_keys: nothing was generated, nothing asked for
    assert np.array_equal(array, V.export(z))
    with pytest.raises(RuntimeError, match="no secret key"):
        S.decrypt(z)
    out = enc.decode_packed(array, meta)                   # the client: one decryption
    assert len(out) == 1 and np.array_equal(out[0], state)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_context_usable(client, members):
    which, C = client
    E = C.engine
    msgs, cts = members[16]
    a, b = cts[0], cts[5]

    def covered():
        z = E.pack_periodic([a, b, None, cts[1], cts[2]], 16)
        assert z.pack == (8, 16) and E.check(z) is None
        E.export(E.stack([a, cts[1]]))

    covered()
    E.sync()
    before = E.pool_stats()["bytes"]
    st = E.stack([a, cts[1]])
    with pytest.raises(RuntimeError, match="member count"):
        E.pack_periodic([], 16)
    with pytest.raises(RuntimeError, match="member count"):
        E.pack_periodic([a] * 33, 16)
    out = ctypes.c_uint64()
    assert E._lib.aesfhe_pack_periodic(E._ctx.ptr, 2, None, 16, ctypes.byref(out)) == -1   # no member array
    with pytest.raises(RuntimeError, match="absent"):
        E.pack_periodic([None, None, None], 16)
    with pytest.raises(RuntimeError, match="stack"):
        E.pack_periodic([a, st], 16)
    for period in (0, -16, 3, 24):
        with pytest.raises(RuntimeError, match="power of two"):
            E.pack_periodic([a, b], period)
    with pytest.raises(RuntimeError, match="exceeds the slot count"):
        E.pack_periodic([a] * 32, 256)                     # G = 32: 8192 > 4096 slots
    with pytest.raises(RuntimeError, match="exceeds the slot count"):
        E.pack_periodic([a, b, b], E.slot_count // 2)      # T = 3 is G = 4
    with pytest.raises(RuntimeError, match="invalid ciphertext handle"):
        E._ctx.check(E._lib.aesfhe_pack_periodic(E._ctx.ptr, 1, (ctypes.c_uint64 * 1)(1 << 60), 16, ctypes.byref(out)))
    assert E.pack_periodic([a, b], E.slot_count // 2).pack == (2, E.slot_count // 2)   # the largest period that fits
    del st
    gc.collect()
    covered()
    E.sync()
    assert E.pool_stats()["bytes"] <= before
