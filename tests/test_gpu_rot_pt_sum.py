"""aesfhe_rot_pt_sum / Engine.rot_pt_sum: the masked rotation sum of one ciphertext,
double-hoisted -- one ModUp, k_rot_mask_mac, one ModDown per output -- against the composed form (rotate,
multiply by the mask, add), both decrypted.

Small set: N = 2^13, max_level 10, dnum 2 -> alpha = 6, n_p = 7.  Level 1 (3 limbs) is a reduced level of the
per-level special basis (4 special primes with the option on, 7 with it off); the fresh level 10 (12 limbs) has
two digits and keeps all 7 either way.

Tolerance: not a constant.  Every case measures the composed form's own decrypted error against the exact numpy
value of the same inputs and allows the fused form 4 x that: the fused form pays one ModDown where the composed
form pays one per rotation, so its error should be no larger, and the factor only covers seed-to-seed spread.
Measured on an MI355X (max slot error over the cases below, fused / composed; the test prints every case, DESIGN.md
§3.18 has the table): level 1: 1.4e-5 .. 2.1e-5 / 1.4e-5 .. 2.6e-5, fresh level: 8.9e-6 .. 1.4e-5 / 8.9e-6 .. 2.7e-5,
pending input: 1.4e-5 .. 1.7e-5 / 1.7e-5 .. 1.9e-5; fused / composed ratio 0.50 .. 1.00 (1.00: the one-term, step-0 case).
One 11-step, 2-output call issues 16 kernel launches, ten aesfhe_rotate calls 100.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOG_N, LMAX, DNUM = 13, 10, 2


@pytest.fixture(scope="module")
def E():
    from mi355x_ckks import Engine
    # defer_calls=False: every call runs when it is made (the composed form is then n separate key switches)
    e = Engine(log_n=LOG_N, max_level=LMAX, dnum=DNUM, seed=0x5C, allow_insecure=True, enc_nonce=0x5C, defer_calls=False)
    assert (e.alpha, e.n_p) == (6, 7)
    return e


def _input(E, level, seed, pending=False):
    rng = np.random.default_rng(seed)
    z = np.exp(2j * np.pi * rng.random(E.slot_count))
    ct = E.encrypt(z)
    if pending:
        # a non-constant plaintext product leaves its rescale owed: the input then arrives one data level up
        w = 0.5 + 0.5 * rng.random(E.slot_count)
        ct = E.level_down(ct, level + 1) if level + 1 < E.fresh_level else ct
        ct = E.multiply(ct, E.encode(w))
        z = z * w
    elif level < E.fresh_level:
        ct = E.level_down(ct, level)
    return ct, z


def _masks(E, rng, n, n_out, absent=()):
    """per output: n slot vectors (None: absent).  0 / 1 cell-style masks for one output, complex values of
    magnitude <= 1 for the other"""
    sc = E.slot_count
    vals = []
    for j in range(n_out):
        row = []
        for i in range(n):
            if (j, i) in absent:
                row.append(None)
            elif j == 0:
                row.append((rng.integers(0, max(n, 2), sc) == i).astype(np.complex128))
            else:
                row.append(rng.random(sc) * np.exp(2j * np.pi * rng.random(sc)))
        vals.append(row)
    return vals


def _both(E, ct, z, steps, vals):
    """(fused error, composed error) per output, each against the exact numpy value"""
    pts = [[None if v is None else E.encode(v) for v in row] for row in vals]
    fused = E.rot_pt_sum(ct, steps, pts)
    assert len(fused) == len(vals)
    errs = []
    for j, row in enumerate(vals):
        want = np.zeros(E.slot_count, np.complex128)
        comp = None
        for s, v, p in zip(steps, row, pts[j]):
            if v is None:
                continue
            want += v * np.roll(z, s)
            term = E.multiply(E.rotate(ct, delta=s), p)
            comp = term if comp is None else E.add(comp, term)
        ef = float(np.abs(E.decrypt(fused[j]) - want).max())
        ec = float(np.abs(E.decrypt(comp) - want).max())
        errs.append((ef, ec))
    return fused, errs


def _shapes(sc):
    return {
        "n1_step0": ([0], 1, ()),
        "n3": ([0, 5, -3], 1, ()),
        # negatives, values at and above slot_count (sc itself is the identity), two outputs, absent terms
        # (the first step, slot_count itself, is the identity: no key switch; the other ten rotate)
        "n11x2": ([sc, 1, -1, 2, -2, 3, -3, sc + 7, -(sc + 9), sc + 5, 2 * sc - 4], 2, ((0, 3), (1, 0), (1, 7), (0, 10))),
    }


@pytest.mark.parametrize("low", [False, True], ids=["fullP", "lowP"])
@pytest.mark.parametrize("level", [1, LMAX], ids=["level1", "fresh"])
def test_matches_composed(E, level, low):
    E.set_low_p(low)
    try:
        assert E.ks_special_primes(1) == (4 if low else 7)
        for k, (name, (steps, n_out, absent)) in enumerate(_shapes(E.slot_count).items()):
            ct, z = _input(E, level, 100 * level + k)
            rng = np.random.default_rng(7 + k)
            fused, errs = _both(E, ct, z, steps, _masks(E, rng, len(steps), n_out, absent))
            for j, (ef, ec) in enumerate(errs):
                print(f"rot_pt_sum {name} level {level} low_p {int(low)} out {j}: fused {ef:.3g}, composed {ec:.3g}, ratio {ef / ec:.2f}")
                assert fused[j].level == level - 1  # the logical level: the data level is the input's, one rescale owed
                assert ef <= 4.0 * ec, (name, level, low, j, ef, ec)
    finally:
        E.set_low_p(False)


@pytest.mark.parametrize("low", [False, True], ids=["fullP", "lowP"])
def test_pending_rescale_input(E, low):
    E.set_low_p(low)
    try:
        ct, z = _input(E, 2, 31, pending=True)
        steps = [0, 4, -6]
        fused, errs = _both(E, ct, z, steps, _masks(E, np.random.default_rng(3), 3, 2))
        for j, (ef, ec) in enumerate(errs):
            print(f"rot_pt_sum pending input low_p {int(low)} out {j}: fused {ef:.3g}, composed {ec:.3g}, ratio {ef / ec:.2f}")
            assert ef <= 4.0 * ec, (j, ef, ec)
    finally:
        E.set_low_p(False)


def test_refusals(E):
    ct, _ = _input(E, 3, 5)
    sc = E.slot_count
    pt = E.encode((np.arange(sc) % 2).astype(np.complex128))
    with pytest.raises(RuntimeError, match="stack"):
        E.rot_pt_sum(E.stack([ct, ct]), [1], [[pt]])
    with pytest.raises(RuntimeError, match="1..16 terms"):
        E.rot_pt_sum(ct, list(range(17)), [[pt] * 17])
    with pytest.raises(RuntimeError, match="1..2 outputs"):
        E.rot_pt_sum(ct, [1], [[pt], [pt], [pt]])
    tensor = E._raw_mul(ct, ct, False)
    with pytest.raises(RuntimeError, match="2-polynomial"):
        E.rot_pt_sum(tensor, [1], [[pt]])
    assert np.abs(E.decrypt(E.rot_pt_sum(ct, [1], [[pt]])[0])).max() < 2.0  # the engine still serves calls


def test_fewer_launches_than_ten_rotations(E):
    import mi355x_ckks
    steps, n_out, absent = _shapes(E.slot_count)["n11x2"]
    ct, _ = _input(E, 3, 11)
    vals = _masks(E, np.random.default_rng(1), len(steps), n_out, absent)
    pts = [[None if v is None else E.encode(v) for v in row] for row in vals]
    rot = [s for s in steps if s % E.slot_count]
    assert len(rot) == 10
    E.rot_pt_sum(ct, steps, pts)          # first calls: rotation keys generated, masks encoded
    for s in rot:
        E.rotate(ct, delta=s)
    n0 = mi355x_ckks.launch_count()
    E.rot_pt_sum(ct, steps, pts)
    n1 = mi355x_ckks.launch_count()
    for s in rot:
        E.rotate(ct, delta=s)
    n2 = mi355x_ckks.launch_count()
    print(f"launches: rot_pt_sum (11 steps, 2 outputs) {n1 - n0}, 10 rotations {n2 - n1}")
    assert n1 - n0 < n2 - n1


def test_mask_encodings_released_with_the_handles(E):
    """the pool's byte count covers buffers in use and buffers cached for reuse, so a released buffer shows
    as NO growth when the same work runs again: after one warm round (masks encoded over Q*P, call made,
    everything freed) a second identical round with new plaintext handles must leave the count where it was.
    Encodings that stayed behind their freed handles would make the second round allocate new ones."""
    import gc

    def round_():
        ct, _ = _input(E, 3, 17)
        steps = [0, 2, -5, 9]
        vals = _masks(E, np.random.default_rng(2), 4, 2)
        pts = [[E.encode(v) for v in row] for row in vals]
        out = E.rot_pt_sum(ct, steps, pts)
        E.decrypt(out[0])
        del ct, pts, out
        gc.collect()

    round_()
    before = E.pool_stats()["bytes"]
    round_()
    assert E.pool_stats()["bytes"] == before
