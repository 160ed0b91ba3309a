"""The three public-operand multiply-accumulate ops pinned bit for bit (tools/public_mac_digest.py against
tests/golden/public_mac_digests.json, recorded at the commit the file names): lut_eval_public, xor_value_public and
xor_value_typed give the same output residues, the same output levels, the same kernel launches and the same
number of rescales inside the call, and the three debug readbacks the same rows.  The oracle-parity and bit-exact
MAC tests (test_gpu_public_lut, test_gpu_xor_value, test_gpu_value_typed) check the ops against an independent
model; these check them against their own past, which also sees an operand normalised differently, a launch more
or a rescale taken on the other side of the headroom test.

Each group of cases runs on an engine of its own, so a group is one test; a failure names the first case that
differs.  The refusals keep their full texts (part of the C ABI's behaviour)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))

import public_mac_digest as pmd  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((ROOT / "tests" / "golden" / "public_mac_digests.json").read_text())


def test_golden_covers_every_group():
    assert sorted(GOLDEN["groups"]) == sorted(pmd.GROUPS)


def test_heavy_weights_rescale_inside_the_call():
    """the golden file itself: the 2^24 weights left no headroom at the parent, the small ones did"""
    typed = GOLDEN["groups"]["typed"]
    assert typed["typed_heavy_rescaled"]["rescale"] == 2
    assert typed["typed_groups1"]["rescale"] == typed["typed_groups2"]["rescale"] == 1  # the one operand that owed its own


@pytest.mark.parametrize("group", list(pmd.GROUPS))
def test_public_mac_bit_identical(group):
    want = GOLDEN["groups"][group]
    got = pmd.group_digests(group)
    assert sorted(got) == sorted(want)
    for name in got:  # in the order the cases ran: the first difference is the one to look at
        assert got[name] == want[name], f"first differing case: {name} (golden of {GOLDEN['parent']})"


def test_validation_messages():
    E = pmd._engine()
    rng = np.random.default_rng(0xA5)
    sc = E.slot_count
    nib, = pmd.nibbles(E, rng)
    bad = nib.copy()
    bad[sc // 2] = 16
    short = nib[:-1].copy()
    tabs = pmd.value_tables(1.0 / 256.0)
    w = np.full((2, sc), 1.0 / 256.0)
    a_hi, a_lo = pmd.flat_powers(E, rng, 3)
    zero_level = {p: pmd.ct(E, 0, rng) for p in range(1, 9)}
    stacked = {**a_hi, 3: E.stack([a_hi[3], a_hi[5]])}
    three = {**a_hi, 2: E._raw_mul(a_hi[1], a_hi[2], relin=False)}
    assert three[2].num_polys == 3
    missing = {p: a_lo[p] for p in range(1, 8)}
    l1, _ = pmd.xor4_luts(E)
    a = {p: a_hi[p] for p in pmd.LUT_ROWS}

    def fails(msg, fn, *args):
        with pytest.raises(RuntimeError) as e:
            fn(*args)
        assert str(e.value) == msg

    def value(who):
        """the refusals xor_value_public and xor_value_typed share, under each one's own prefix"""
        def call(hi, lo, nh, nl):
            return E.xor_value_public(hi, lo, nh, nl, *tabs) if who == "xor_value_public" else E.xor_value_typed(hi, lo, nh, nl, w[:, :nh.size])
        fails(f"{who}: missing element handle of a used row", call, a_hi, missing, nib, nib)
        fails(f"{who}: stacked operands are not supported (single ciphertexts only)", call, stacked, a_lo, nib, nib)
        fails(f"{who}: nonzero 2-polynomial ciphertexts", call, three, a_lo, nib, nib)
        fails(f"{who}: one nibble per slot (n_slots must equal slot_count)", call, a_hi, a_lo, short, short)
        fails(f"{who}: nibble out of range (>= 16) at slot {sc // 2}", call, a_hi, a_lo, nib, bad)
        fails(f"{who}: nibble out of range (>= 16) at slot {sc // 2}", call, a_hi, a_lo, bad, nib)
        return call

    call = value("xor_value_public")
    fails("not enough level for the public value decode (level 0)", call, zero_level, a_lo, nib, nib)
    call = value("xor_value_typed")
    fails("not enough level for the typed value decode (level 0)", call, zero_level, a_lo, nib, nib)
    fails("xor_value_typed: n_groups must be 1 or 2", E.xor_value_typed, a_hi, a_lo, nib, nib, np.ones((3, sc)))
    fails("xor_value_typed: missing weights", E.xor_value_typed, a_hi, a_lo, nib, nib, None)  # a null pointer at the C entry
    for poison in (np.nan, np.inf):
        wb = w.copy()
        wb[1, sc - 1] = poison
        fails(f"xor_value_typed: weight not finite at group 1, slot {sc - 1}", E.xor_value_typed, a_hi, a_lo, nib, nib, wb)
    # a bad weight is reported before a bad nibble, a bad slot count before either
    wb = w.copy()
    wb[0, 7] = np.nan
    fails("xor_value_typed: weight not finite at group 0, slot 7", E.xor_value_typed, a_hi, a_lo, nib, bad, wb)

    fails("lut_eval_public: missing element handle of a used row", E.lut_eval_public, l1, None, {1: a[1]}, nib)
    fails("lut_eval_public: stacked operands are not supported (single ciphertexts only)", E.lut_eval_public, l1, None,
          {**a, 3: stacked[3]}, nib)
    fails("lut_eval_public: nonzero 2-polynomial ciphertexts", E.lut_eval_public, l1, None, {**a, 3: three[2]}, nib)
    fails("not enough level for the public-operand LUT (level 0)", E.lut_eval_public, l1, None, {**a, 5: zero_level[5]}, nib)
    fails("lut_eval_public: one nibble per slot (n_slots must equal slot_count)", E.lut_eval_public, l1, None, a, short)
    fails(f"lut_eval_public: nibble out of range (>= 16) at slot {sc // 2}", E.lut_eval_public, l1, None, a, bad)

    top = E.max_level + 1
    fails("debug_xor_value_pt: level out of range (1..max level)", E.debug_xor_value_pt, nib, nib, *tabs, 0)
    fails("xor_value_public: nibble out of range (>= 16) at slot 0", E.debug_xor_value_pt, np.full(sc, 16, np.uint8), nib, *tabs, 3)
    fails("debug_xor_value_typed_pt: n_groups must be 1 or 2", E.debug_xor_value_typed_pt, nib, nib, np.ones((3, sc)), None, 3)
    fails("debug_xor_value_typed_pt: missing weights", E.debug_xor_value_typed_pt, nib, nib, None, None, 3)
    fails("debug_xor_value_typed_pt: level out of range (1..max level)", E.debug_xor_value_typed_pt, nib, nib, w, None, 0)
    fails("xor_value_typed: weight not finite at group 1, slot 0", E.debug_xor_value_typed_pt, nib, nib, w * [[1.0], [np.inf]], None, 3)
    fails("debug_public_pt: level out of range (1..max level)", E.debug_public_pt, l1, nib, 0)
    fails("lut_eval_public: one nibble per slot (n_slots must equal slot_count)", E.debug_public_pt, l1, short, 3)

    # nothing above changed the operands or leaked: every op still runs on the same handles, at the pool size a first
    # round of the three ops left
    def run_all():
        T, R = E.xor_value_public(a_hi, a_lo, nib, nib, *tabs)
        out = E.xor_value_typed(a_hi, a_lo, nib, nib, w)
        o1, _ = E.lut_eval_public(l1, None, a, nib)
        assert [c.level for c in (T, R, o1)] + [c.level for pr in out for c in pr] == [2] * 7

    run_all()
    E.sync()
    held = E.pool_stats()["bytes"]
    fails("xor_value_typed: weight not finite at group 0, slot 7", E.xor_value_typed, a_hi, a_lo, nib, bad, wb)
    fails("lut_eval_public: nibble out of range (>= 16) at slot 0", E.lut_eval_public, l1, None, a, np.full(sc, 16, np.uint8))
    run_all()
    E.sync()
    assert E.pool_stats()["bytes"] == held
