"""aesfhe_rot_pt_affine / Engine.rot_pt_affine: aesfhe_rot_pt_sum's masked rotation sum plus one fill
plaintext per output, added inside the sum's kernel (k_rot_mask_mac's FILL variant) at the product scale.

The small set of tests/test_gpu_rot_pt_sum.py: N = 2^13, max_level 10, dnum 2 -> alpha = 6, n_p = 7.  Every case runs at
level 2 (4 limbs, one more than the lowest level a plaintext product allows), a reduced level of the per-level special
basis: 5 special primes with the option on, 7 with it off.  (A set of at most 6 levels at dnum 2 has alpha = 4: level
2 would keep the full basis either way and the low-P cases would repeat the others.)

Tolerance: not a constant.  The parent path -- rot_pt_sum, its owed rescale settled, the fill added in clear after
decryption -- runs on the same inputs against the same numpy model sum_i mask_i * np.roll(z, s_i) + fill, and the
affine entry may show at most 2 x its largest slot error: the fill adds ONE plaintext rounding (at the product scale,
~2^-60 relative) to a sum that already carries n of them at the mask scale.  Measured on an MI355X (the test prints
every case): affine 1.2e-5 .. 1.7e-5, parent 1.4e-5 .. 1.8e-5, ratio 0.69 .. 1.08 over the 12 outputs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_N, LMAX, DNUM = 13, 10, 2
LEVEL = 2


@pytest.fixture(scope="module")
def E():
    from mi355x_ckks import Engine
    e = Engine(log_n=LOG_N, max_level=LMAX, dnum=DNUM, seed=0x5C, allow_insecure=True, enc_nonce=0x5C, defer_calls=False)
    assert (e.alpha, e.n_p) == (6, 7)
    return e


def _case(E, n, n_out, seed):
    """(ct, z, steps, mask values per output, fill values per output): 0 / 1 masks that leave slots uncovered, a
    step-0 term first, one absent term where there is room, fills of codeword-like unit values on the rest"""
    rng = np.random.default_rng(seed)
    sc = E.slot_count
    z = np.exp(2j * np.pi * rng.random(sc))
    ct = E.level_down(E.encrypt(z), LEVEL)
    steps = [0, 3, -5, 16, -16, 7, sc - 1, -(sc + 9)][:n]
    vals, fills = [], []
    for j in range(n_out):
        owner = rng.integers(0, n + 1, sc)  # n: no mask covers the slot
        row = [(owner == i).astype(np.complex128) for i in range(n)]
        if n > 1:
            gone = 1 + j  # an absent term: its slots join the fill
            owner[owner == gone] = n
            row[gone] = None
        vals.append(row)
        fills.append(np.where(owner == n, np.exp(2j * np.pi * rng.integers(0, 16, sc) / 16), 0))
    return ct, z, steps, vals, fills


def _model(z, steps, row, fill):
    want = np.zeros(z.shape, np.complex128)
    for s, v in zip(steps, row):
        if v is not None:
            want += v * np.roll(z, s)
    return want + (0 if fill is None else fill)


def _pts(E, vals):
    return [[None if v is None else E.encode(v) for v in row] for row in vals]


@pytest.mark.parametrize("low", [False, True], ids=["fullP", "lowP"])
def test_no_fill_is_rot_pt_sum_bit_for_bit(E, low):
    E.set_low_p(low)
    try:
        for n, n_out in ((1, 1), (8, 2)):
            ct, _, steps, vals, _ = _case(E, n, n_out, 40 + n)
            pts = _pts(E, vals)
            a = E.rot_pt_affine(ct, steps, pts, [None] * n_out)
            b = E.rot_pt_sum(ct, steps, pts)
            for x, y in zip(a, b):
                assert x.level == y.level == LEVEL - 1
                assert np.array_equal(E.export(x), E.export(y))
    finally:
        E.set_low_p(False)


@pytest.mark.parametrize("low", [False, True], ids=["fullP", "lowP"])
@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("n", [1, 8])
def test_fill_matches_the_model_within_twice_the_parent_error(E, n, n_out, low):
    E.set_low_p(low)
    try:
        assert E.ks_special_primes(LEVEL) == (5 if low else 7)
        ct, z, steps, vals, fills = _case(E, n, n_out, 10 * n + n_out)
        pts = _pts(E, vals)
        fl = [E.encode(f) for f in fills]
        if n_out == 2:
            fl[1], fills[1] = None, None  # one output with a fill beside one without
        got = E.rot_pt_affine(ct, steps, pts, fl)
        parent = E.rot_pt_sum(ct, steps, pts)
        for j in range(n_out):
            want = _model(z, steps, vals[j], fills[j])
            assert got[j].level == LEVEL - 1  # owes its rescale, as rot_pt_sum's output
            ea = float(np.abs(E.decrypt(got[j]) - want).max())
            settled = E.level_down(parent[j], parent[j].level)  # the owed rescale applied
            ep = float(np.abs(E.decrypt(settled) + (0 if fills[j] is None else fills[j]) - want).max())
            print(f"rot_pt_affine n {n} n_out {n_out} low_p {int(low)} out {j} fill {int(fills[j] is not None)}: "
                  f"affine {ea:.3g}, parent {ep:.3g}, ratio {ea / ep:.2f}")
            assert ea <= 2.0 * ep, (n, n_out, low, j, ea, ep)
    finally:
        E.set_low_p(False)


def test_refusals_and_fill_encodings_released(E):
    import gc
    ct, _, steps, vals, fills = _case(E, 8, 1, 77)
    pts, fl = _pts(E, vals), [E.encode(fills[0])]
    with pytest.raises(RuntimeError, match="stack"):
        E.rot_pt_affine(E.stack([ct, ct]), steps, pts, fl)
    with pytest.raises(RuntimeError, match="1..2 outputs"):
        E.rot_pt_affine(ct, steps, pts * 3, fl * 3)
    with pytest.raises(ValueError):
        E.rot_pt_affine(ct, steps, pts, [])

    def round_():
        c, _, st, v, f = _case(E, 8, 2, 78)
        out = E.rot_pt_affine(c, st, _pts(E, v), [E.encode(x) for x in f])
        E.decrypt(out[1])
        del c, out
        gc.collect()

    round_()
    before = E.pool_stats()["bytes"]
    round_()
    assert E.pool_stats()["bytes"] == before  # the fills' encodings went back with their handles
