"""EvaluationKeys (evaluation_keys.py): the bundle a client hands a server -- save / load round trip
on synthetic arrays, header validation, and that nothing named for a secret or a seed reaches the disk.  No engine."""
import json

import numpy as np
import pytest

LOG_N, N_Q, N_P = 4, 3, 2
N = 1 << LOG_N
MODULI = [97, 193, 257, 353, 449]


def _header(**over):
    from evaluation_keys import make_header
    kw = dict(log_n=LOG_N, max_level=1, dnum=2, bootstrappable=False, low_p=True, n_q=N_Q, n_p=N_P, moduli=MODULI)
    kw.update(over)
    return make_header(**kw)


def _arrays(seed=0):
    rng = np.random.default_rng(seed)
    pk = rng.integers(0, 97, 2 * N_Q * N, dtype=np.uint32)
    keys = {(0, -1): rng.integers(0, 97, 2 * 2 * (N_Q + N_P) * N, dtype=np.uint32),
            (2 * N - 1, -1): rng.integers(0, 97, 2 * 2 * (N_Q + N_P) * N, dtype=np.uint32),
            (5, 0): rng.integers(0, 97, 2 * 5 * N, dtype=np.uint32)}
    return pk, keys


def test_save_load_round_trip(tmp_path):
    from evaluation_keys import EvaluationKeys
    pk, keys = _arrays()
    b = EvaluationKeys(_header(), pk, keys)
    assert b.key_ids() == sorted(keys)
    written = b.save(tmp_path / "bundle")
    assert written == pk.nbytes + sum(v.nbytes for v in keys.values()) == b.nbytes()
    r = EvaluationKeys.load(tmp_path / "bundle")
    assert r.header == b.header and r.key_ids() == b.key_ids()
    assert np.array_equal(r.pk, pk) and isinstance(r.pk, np.memmap)
    for k, v in r.items():
        assert isinstance(v, np.memmap) and v.dtype == np.uint32 and np.array_equal(v, keys[k])


def test_streamed_bundle_saves_key_by_key(tmp_path):
    """an iterator of keys is consumed one at a time through ONE reused buffer: what is on disk is each key's own
    content, so save never kept a reference to an earlier key"""
    from evaluation_keys import EvaluationKeys
    pk, keys = _arrays(1)
    buf = np.zeros(max(v.size for v in keys.values()), np.uint32)
    live = []

    def produce():
        for k in sorted(keys):
            live.append(k)
            assert len(live) == 1  # the consumer took the previous key before asking for this one
            buf[:keys[k].size] = keys[k]
            yield k, buf[:keys[k].size]
            live.pop()

    b = EvaluationKeys(_header(), pk, produce())
    with pytest.raises(ValueError, match="streamed"):
        b.key_ids()
    b.save(tmp_path)
    r = EvaluationKeys.load(tmp_path)
    for k in keys:
        assert np.array_equal(r[k], keys[k])
    with pytest.raises(ValueError, match="consumed"):
        list(b.items())


def test_header_validation(tmp_path):
    from evaluation_keys import EvaluationKeys
    pk, keys = _arrays(2)
    with pytest.raises(ValueError, match="version"):
        EvaluationKeys(dict(_header(), version=2), pk, keys)
    with pytest.raises(ValueError, match="moduli"):
        EvaluationKeys(dict(_header(), moduli=MODULI[:-1]), pk, keys)
    with pytest.raises(ValueError, match="moduli"):
        _header(n_p=N_P + 1)
    with pytest.raises(ValueError, match="duplicate"):
        list(EvaluationKeys(_header(), pk, iter([((0, -1), keys[(0, -1)]), ((0, -1), keys[(0, -1)])])).items())
    with pytest.raises(ValueError, match="low_p off"):
        EvaluationKeys(_header(low_p=False), pk, keys)
    with pytest.raises(ValueError, match="public key"):
        EvaluationKeys(_header(), pk[:-1], keys)
    with pytest.raises(ValueError, match="uint32"):
        EvaluationKeys(_header(), pk, {(0, -1): keys[(0, -1)].astype(np.int64)})
    # the same checks on what load reads
    EvaluationKeys(_header(), pk, keys).save(tmp_path)
    doc = json.loads((tmp_path / "header.json").read_text())
    for bad, match in ((dict(doc, header=dict(doc["header"], version=7)), "version"),
                       (dict(doc, keys=doc["keys"] + [doc["keys"][0]]), "duplicate"),
                       (dict(doc, header=dict(doc["header"], low_p=False)), "low_p off"),
                       (dict(doc, header=dict(doc["header"], secret=[1])), "unknown header fields")):
        (tmp_path / "header.json").write_text(json.dumps(bad))
        with pytest.raises(ValueError, match=match):
            EvaluationKeys.load(tmp_path)


def test_nothing_named_for_a_secret_or_a_seed_on_disk(tmp_path):
    from evaluation_keys import HEADER_FIELDS, EvaluationKeys
    pk, keys = _arrays(3)
    EvaluationKeys(_header(), pk, keys).save(tmp_path)
    words = ("secret", "seed", "prng", "sparse", "sk")
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted(["header.json", "pk.npy"] + [f"ksk_{g}_{'full' if l < 0 else l}.npy" for g, l in keys])
    doc = json.loads((tmp_path / "header.json").read_text())
    fields = set(doc) | set(doc["header"])
    assert set(doc["header"]) == set(HEADER_FIELDS)
    for w in words:
        assert not any(w in n.lower().replace("ksk", "") for n in names), w
        assert not any(w in f.lower() for f in fields), w
