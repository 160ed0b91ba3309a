"""The secret-key renorm pinned bit for bit (tools/renorm_digest.py against tests/golden/renorm_digests.json,
recorded at the commit the file names): every shape, codec and re-encryption path gives the same output
residues, the same output levels and the same kernel launches.  The slot-tolerance tests of the renorm
(test_gpu_renorm_pool, test_gpu_conj_renorm, ...) would pass a swapped codec, a lost accumulator flip or an
encryption counter consumed out of order; these do not.

Each group of cases runs on an engine of its own (the encryption counter never resets), so a group is one
test; a failure names the first case that differs.

The validation failures keep their messages (part of the C ABI's behaviour).  Two of the renorm's checks
cannot be reached through the C ABI and are not called here: a conjugate partner on the lo channel of a
one-input renorm and a one-input renorm reading two ciphertexts (no entry point passes either)."""
import ctypes
import json
import sys
import types
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))

import renorm_digest  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((ROOT / "tests" / "golden" / "renorm_digests.json").read_text())


def test_golden_covers_every_group():
    assert sorted(GOLDEN["groups"]) == sorted(renorm_digest.GROUPS)


@pytest.mark.parametrize("group", list(renorm_digest.GROUPS))
def test_renorm_bit_identical(group):
    want = GOLDEN["groups"][group]
    got = renorm_digest.group_digests(group)
    assert sorted(got) == sorted(want)
    for name in got:  # in the order the cases ran: the first difference is the one to look at
        assert got[name] == want[name], f"first differing case: {name} (golden of {GOLDEN['parent']})"


def test_validation_messages():
    E = renorm_digest._engine()
    S = E.slot_count
    h, l, x = (renorm_digest._noisy(E, p, s) for p, s in ((16, 1), (16, 2), (32, 3)))
    st3, st2 = E.stack([h, l, h]), E.stack([h, l])
    none = types.SimpleNamespace(handle=0)
    bad = list(renorm_digest.SR)
    bad[5] = 16

    def fails(msg, fn, *a, **k):
        with pytest.raises(RuntimeError) as e:
            fn(*a, **k)
        assert str(e.value) == msg

    fails("renorm: bad period", E.renorm_periodic, h, l, 24)
    fails("renorm: bad period", E.renorm_periodic, h, l, 2 * S)
    fails("renorm: bad packed period", E.renorm_unpack, x, 24)
    fails("renorm: bad packed period", E.renorm_unpack, x, S)
    fails("renorm: states per ciphertext must be in [1, slot_count / 16]", E.renorm_pair, h, l, S // 16 + 1)
    fails("renorm: states per ciphertext must be in [1, slot_count / 16]", E.renorm_pair, h, l, 0, E.max_level)
    fails("renorm: hi and lo stacks of different sizes", E.renorm_periodic, st3, st2, 16)
    fails("renorm: a slot permutation needs a single period-16 state pair", E.renorm_periodic_perm, st2, st2, 16, renorm_digest.SR)
    fails("renorm: a slot permutation needs a single period-16 state pair", E.renorm_periodic_perm, h, l, 32, renorm_digest.SR)
    fails("renorm: slot permutation entries must lie in [0, 16)", E.renorm_periodic_perm, h, l, 16, bad)
    fails("renorm: slot permutation entries must lie in [0, 16)", E.renorm_unpack_perm, x, 16, bad)
    fails("renorm: the packed output needs a single period-16 state pair", E.renorm_pack, h, l, 32)
    fails("renorm: conjugate partners: one per input channel", E.renorm_periodic, h, l, 16, None, conj=(h, none))
    fails("renorm: conjugate partners: one per input channel", E.renorm_periodic, h, l, 16, None, conj=(none, l))
    fails("renorm_periodic_perm: give both conjugate partners or none", E.renorm_periodic_perm, h, l, 16, renorm_digest.SR, None,
          conj=(h, none))
    fails("renorm_pack: give both conjugate partners or none", E.renorm_pack, h, l, 16, None, conj=(none, l))
    fails("renorm_packed: period must be a power of two >= 16", E.renorm_single, x, None, period=24)
    # a null permutation: the entry points through a second view of the library that takes a raw pointer
    L = ctypes.CDLL(E._lib._name)
    out = (ctypes.c_uint64 * 2)()
    H, ptr = ctypes.c_uint64, E._ctx.ptr
    assert L.aesfhe_renorm_periodic_perm(ptr, H(h.handle), H(l.handle), H(0), H(0), None, 0, 16, -1, out, ctypes.byref(out, 8)) != 0
    assert E._lib.aesfhe_last_error(ptr).decode() == "renorm_periodic_perm: no permutation"
    assert L.aesfhe_renorm_unpack_perm(ptr, H(x.handle), H(0), None, 16, -1, out, ctypes.byref(out, 8)) != 0
    assert E._lib.aesfhe_last_error(ptr).decode() == "renorm_unpack_perm: no permutation"
    # nothing above changed the engine's state: a renorm still runs
    gh, gl = E.renorm_periodic(h, l, 16)
    assert gh.level == gl.level == E.max_level
    assert np.isfinite(E.decrypt(gh)).all()
