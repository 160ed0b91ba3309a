"""The logged run is the run: one middle encrypt round with a debug dict issues the engine calls of
the same round without one, plus the decodes of its snapshots and nothing else -- in the secret-key renorm mode on the
pair steps and on the packed path, and in true-FHE mode.

What a decode moves depends on the state of the ciphertext it reads (a snapshot taken before the next step's deferred
rescale decrypts over more limbs than a clean one), so each log call of the logged round is counted where it happens,
alone, on the very snapshot it takes: the logged round equals the unlogged round plus exactly those counts."""
import numpy as np
import pytest

from conftest import gpu_context

pytestmark = pytest.mark.gpu

MODES = {
    "pair-steps": dict(use_hard_renorm_between_steps=True, packed_xor=False),
    "packed": dict(use_hard_renorm_between_steps=True),
    "true-fhe": dict(use_hard_renorm_between_steps=False, true_fhe=True),
}


@pytest.fixture(scope="module")
def ctx():
    return gpu_context(log_n=16, signature=1)  # the set of test_gpu_reference_paths.py and test_gpu_bootstrap.py


def _moved(ctx, fn):
    """(fn(), what it moved: the engine counters and the renorm tally, as differences)"""
    from utils import RENORM_TALLY
    E = ctx.engine
    E.sync()
    c0, t0 = E.counters(), dict(RENORM_TALLY)
    out = fn()
    E.sync()
    c1 = E.counters()
    moved = {k: c1[k] - c0[k] for k in c1}
    moved.update({"renorm." + k: RENORM_TALLY[k] - t0[k] for k in t0})
    return out, moved


@pytest.mark.parametrize("mode", sorted(MODES))
def test_debug_round_issues_the_unlogged_rounds_engine_calls(ctx, coeff_dir, mode):
    from aes_keyschedule import expand_aes128_key, load_all_coeffs
    from oracle import aes_plain as A
    from pipeline import AESPipeline
    pipe = AESPipeline(ctx, load_all_coeffs(coeff_dir), **MODES[mode])
    assert pipe.packed_xor == (mode == "packed")
    rng = np.random.default_rng(0x109)
    rks = expand_aes128_key(rng.integers(0, 256, 16).astype(np.uint8))
    pt = rng.integers(0, 256, 16).astype(np.uint8)
    want = A.ref_mix_columns(A.shift_rows(A.SBOX[pt ^ rks[0]])) ^ rks[1]
    rk = pipe._prepare_round_keys(rks)

    def round_input():
        """equal inputs: the same bytes through the same steps, settled, and the renorm's pools of zero encryptions
        emptied at their default size, so that both counted rounds refill them alike"""
        ct = pipe._ark_renorm(pipe.encoder.encode(pt), rk[0], level=pipe.need_sub)
        ctx.engine.settle(*ct)
        ctx.engine.renorm_pool(16)
        return ct

    # the counters a snapshot's decode moves, measured on a clean pair and a clean packed state, alone
    clean = round_input()
    _, pair_cost = _moved(ctx, lambda: pipe._log_pair({}, "pair", *clean))
    only = {k for k, v in pair_cost.items() if v}
    per_stage = [pair_cost["decrypt"]] * 6
    if pipe.packed_xor:
        packed = pipe.encoder.encode_packed(pt)
        _, packed_cost = _moved(ctx, lambda: pipe._log_packed({}, "packed", packed))
        only |= {k for k, v in packed_cost.items() if v}
        per_stage[2:5] = [packed_cost["decrypt"]] * 3  # sr, mc and ark are single packed ciphertexts
    assert "decrypt" in only and only <= {"decrypt", "ntt_rows"}, only

    pipe.encrypt_round(round_input(), rk[1], {}, 1)  # every cache filled, those of the snapshot decodes included
    ct = round_input()
    plain_out, plain = _moved(ctx, lambda: pipe.encrypt_round(ct, rk[1], None, 1))
    # the logged round, each of its log calls counted alone where it happens.  A snapshot the deferred-call layer has
    # not issued yet (deferred_calls.Deferred) is resolved first: the decode would resolve it anyway, and so would the
    # next step of the unlogged round, so that work belongs to the round and not to the log call
    from deferred_calls import Deferred
    spent = {k: 0 for k in plain}

    def counted(log):
        def call(dbg, tag, *cts, **meta):
            for c in cts:
                if isinstance(c, Deferred):
                    c.resolved()
            _, m = _moved(ctx, lambda: log(dbg, tag, *cts, **meta))
            for k in spent:
                spent[k] += m[k]
        return call

    pipe._log_pair, pipe._log_packed = counted(pipe._log_pair), counted(pipe._log_packed)
    ct, dbg = round_input(), {}
    logged_out, logged = _moved(ctx, lambda: pipe.encrypt_round(ct, rk[1], dbg, 1))
    del pipe._log_pair, pipe._log_packed
    assert list(dbg) == [f"enc.r1.{s}" for s in ("sub", "sub.renorm", "sr", "mc", "ark", "ark.renorm")]
    assert all(e["plain"] is not None for e in dbg.values()), {t: e.get("plain_err") for t, e in dbg.items()}
    print(f"\n{mode}: unlogged  {plain}\n{mode}: logged    {logged}\n{mode}: log calls {spent}\n{mode}: one clean pair decoded {pair_cost}")
    # the log calls move only what a decode moves, one clean decode's decryptions per logged stage ...
    assert not any(v for k, v in spent.items() if k not in only), spent
    assert spent["decrypt"] == sum(per_stage), (spent["decrypt"], per_stage)
    # ... and the logged round is the unlogged round plus exactly that, in every counter
    diff = {k: (logged[k], plain[k], spent[k]) for k in plain if logged[k] != plain[k] + spent[k]}
    assert not diff, diff  # {counter: (the logged round, the unlogged round, the log calls)}
    assert plain["renorm.calls"] + plain["bootstrap"] > 0 and plain["mul"] + plain["lut"] > 0  # the counters saw the round
    assert plain_out[0].level == logged_out[0].level and plain_out[1].level == logged_out[1].level
    assert np.array_equal(pipe.encoder.decode(*plain_out), want)
    assert np.array_equal(pipe.encoder.decode(*logged_out), want)
    assert np.array_equal(dbg["enc.r1.ark.renorm"]["plain"], want)
