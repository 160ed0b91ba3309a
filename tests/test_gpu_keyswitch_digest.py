"""The complete key switch pinned bit for bit (tools/keyswitch_digest.py against tests/golden/keyswitch_digests.json,
recorded at the commit the file names): every operation of tests/helpers/keyswitch_ops.py -- relinearisation alone
and fused with its rescale, products relinearised from their factors, rotations, conjugations of canonical, deferred
and lazy three-polynomial ciphertexts, stacks wider than one key-switch chunk, a sparse bootstrap -- gives the same
exported residues, the same levels, the same number of kernel launches and the same engine counters, under every
setting of AESFHE_FUSED_KI x AESFHE_CONJ_REV (log N 13) and of AESFHE_BX_COLS (log N 16).

The A/B tests (test_gpu_fused_ki, test_gpu_conj_rev, test_gpu_bx_cols) compare two settings of one build with each
other; these compare each setting with its own past, which also sees a launch more or a counter less.  One engine
per case, so a case is one test; a failure names the first operation that differs.

The hoisted and accumulating key switches (csrc/engine.hip Hoist, giant_accumulate_many) are pinned the same way by
the second list, hoisted_operations, against tests/golden/hoisted_digests.json: hoisted rotations with a zero step
and a repeat, one galois_multi call over shared, stacked, gathered and lower-level sources, rot_pt_sum / rot_pt_affine,
and the full-slot, sparse and paired sparse bootstraps -- by default and with each of AESFHE_S2D_TRACE,
AESFHE_GIANT_BATCH, AESFHE_FUSED_GIANT, AESFHE_FUSED_BABY, AESFHE_DOUBLE_HOIST off (log N 13), and the log N 16
bootstraps whose groups take the fused-core giant steps.

The ciphertext x ciphertext products (csrc/engine.hip mul, mul_many) are the third list, product_operations, against
tests/golden/product_digests.json: single, squared, level-dropped, deferred and stacked operands (within and beyond one
key-switch chunk), the unrelinearised and the lazy product, multiply_many of one pair, several, more than a group, two
levels, shared level drops, a squared pair and a stacked operand, the power basis, and on the bootstrappable engine
the full-slot and sparse bootstraps (EvalMod's 2 P - 1) and a square at the first double-prime level -- by default and
with each of AESFHE_FUSED_TENSOR, AESFHE_FUSED_RESCALE, AESFHE_BATCH_OPS, AESFHE_FUSED_AFFINE off."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))

import keyswitch_digest as ksd  # noqa: E402
from keyswitch_ops import hoisted_operations, operations, product_operations  # noqa: E402  (tests/helpers: the tool put it on the path)

GOLDEN = json.loads((ROOT / "tests" / "golden" / "keyswitch_digests.json").read_text())
HOISTED = json.loads((ROOT / "tests" / "golden" / "hoisted_digests.json").read_text())
PRODUCTS = json.loads((ROOT / "tests" / "golden" / "product_digests.json").read_text())


def test_golden_covers_every_case():
    """no GPU: the golden file holds every case the tool defines, and each case every operation of the shared list
    that its engine runs (the bootstrap only where the engine has one)"""
    import inspect
    import re
    assert sorted(GOLDEN["cases"]) == sorted(ksd.CASES)
    ops = re.findall(r'yield "(\w+)"', inspect.getsource(operations))
    assert len(ops) == 12 and ops[-1] == "bootstrap_sparse32"
    for case, (_, sparse, _) in ksd.CASES.items():
        rec = GOLDEN["cases"][case]
        assert sorted(rec) == sorted(ops if sparse else ops[:-1]), case
        for name, r in rec.items():
            assert sorted(r) == ["counters", "launches", "level", "sha256"] and r["launches"] > 0, (case, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ksd.CASES))
def test_keyswitch_bit_identical(case):
    want = GOLDEN["cases"][case]
    got = ksd.case_digests(case)
    assert sorted(got) == sorted(want)
    for name in got:  # in the order the operations ran: the first difference is the one to look at
        assert got[name] == want[name], f"first differing operation: {name} (golden of {GOLDEN['parent']})"


def test_hoisted_golden_covers_every_case():
    """no GPU: the second golden file holds every case of the hoisted list, each case every operation its engine runs
    (the bootstraps only where the engine has one; the log N 16 cases the two bootstraps alone), and the record itself
    shows that each switch reaches a path of its own: its case differs from the default's in a launch count"""
    import inspect
    import re
    assert HOISTED["parent"] == "3e58fd4" and sorted(HOISTED["cases"]) == sorted(ksd.HOISTED_CASES)
    ops = re.findall(r'yield "(\w+)"', inspect.getsource(hoisted_operations))[2:]  # after the two of boot == "only"
    assert len(ops) == 8 and ops[5:] == ["bootstrap", "bootstrap_sparse32", "bootstrap_pair_sparse32"]
    for case, (_, boot, _) in ksd.HOISTED_CASES.items():
        rec = HOISTED["cases"][case]
        assert sorted(rec) == sorted(ops[5:7] if boot == "only" else ops if boot else ops[:5]), case
        for name, r in rec.items():
            assert sorted(r) == ["counters", "launches", "level", "sha256"] and r["launches"] > 0, (case, name)
    launches = {c: {n: r["launches"] for n, r in rec.items()} for c, rec in HOISTED["cases"].items()}
    for sw in ("s2d_trace", "giant_batch", "fused_baby", "double_hoist"):
        assert launches[f"n13_boot_{sw}0"] != launches["n13_boot"], sw
    assert launches["n16_boot_fused_giant0"] != launches["n16_boot"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ksd.HOISTED_CASES))
def test_hoisted_bit_identical(case):
    want = HOISTED["cases"][case]
    got = ksd.case_digests(case, "hoisted")
    assert sorted(got) == sorted(want)
    for name in got:  # in the order the operations ran: the first difference is the one to look at
        assert got[name] == want[name], f"first differing operation: {name} (golden of {HOISTED['parent']})"


def test_product_golden_covers_every_case():
    """no GPU: the third golden file holds every case of the product list, each case every operation its engine runs
    (the bootstraps and the double-prime square only on the bootstrappable engine), and the record itself shows that
    each switch reaches a path of its own: its case differs from its engine's default in a launch count"""
    import inspect
    import re
    assert PRODUCTS["parent"] == "6534c24" and sorted(PRODUCTS["cases"]) == sorted(ksd.PRODUCT_CASES)
    ops = re.findall(r'yield "(\w+)"', inspect.getsource(product_operations))
    assert len(ops) == 19 and ops[16:] == ["bootstrap", "bootstrap_sparse32", "mul_squared_boundary"]
    for case, (_, boot, _) in ksd.PRODUCT_CASES.items():
        rec = PRODUCTS["cases"][case]
        assert sorted(rec) == sorted(ops if boot else ops[:16]), case
        for name, r in rec.items():
            assert sorted(r) == ["counters", "launches", "level", "sha256"] and r["launches"] > 0, (case, name)
    launches = {c: {n: r["launches"] for n, r in rec.items()} for c, rec in PRODUCTS["cases"].items()}
    for case in ksd.PRODUCT_CASES:
        default = case[:len("n13_deep")]  # n13_deep / n13_boot
        assert case == default or launches[case] != launches[default], case


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ksd.PRODUCT_CASES))
def test_product_bit_identical(case):
    want = PRODUCTS["cases"][case]
    got = ksd.case_digests(case, "products")
    assert sorted(got) == sorted(want)
    for name in got:  # in the order the operations ran: the first difference is the one to look at
        assert got[name] == want[name], f"first differing operation: {name} (golden of {PRODUCTS['parent']})"
