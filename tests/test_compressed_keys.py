"""CompressedEvaluationKeys (evaluation_keys.py): the bundle of b halves plus the public mask key --
save / load round trip on synthetic arrays, header validation, each loader refusing the other format, load_bundle's
dispatch, the file names, and that nothing named for a secret reaches the disk.  Also pins tests/helpers/mask_prf.py,
the numpy model of the PRF the a halves come from, against the oracle's ChaCha20 block function.  No engine."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))

LOG_N, N_Q, N_P = 4, 3, 2
N = 1 << LOG_N
MODULI = [97, 193, 257, 353, 449]
MASK = bytes(range(0x40, 0x60))


def _params(**over):
    kw = dict(log_n=LOG_N, max_level=1, dnum=2, bootstrappable=False, low_p=True, n_q=N_Q, n_p=N_P, moduli=MODULI)
    kw.update(over)
    return kw


def _header(mask_key=MASK, **over):
    from evaluation_keys import make_compressed_header
    return make_compressed_header(mask_key=mask_key, **_params(**over))


def _halves(seed=0):
    """b halves: [n_q][N], two full keys [dnum][nkey][N], one reduced-level key [nkey_l][N]"""
    rng = np.random.default_rng(seed)
    pk = rng.integers(0, 97, N_Q * N, dtype=np.uint32)
    keys = {(0, -1): rng.integers(0, 97, 2 * (N_Q + N_P) * N, dtype=np.uint32),
            (2 * N - 1, -1): rng.integers(0, 97, 2 * (N_Q + N_P) * N, dtype=np.uint32),
            (5, 0): rng.integers(0, 97, 5 * N, dtype=np.uint32)}
    return pk, keys


def _file_names(keys):
    return sorted(["header.json", "pk_b.npy"] + [f"ksk_{g}_{'full' if l < 0 else l}_b.npy" for g, l in keys])


def test_save_load_round_trip(tmp_path):
    from evaluation_keys import COMPRESSED_FORMAT_VERSION, CompressedEvaluationKeys
    pk, keys = _halves()
    b = CompressedEvaluationKeys(_header(), pk, keys)
    assert b.header["version"] == COMPRESSED_FORMAT_VERSION == 2 and b.header["mask_key"] == MASK.hex() and b.mask_key == MASK
    assert b.key_ids() == sorted(keys)
    written = b.save(tmp_path / "bundle")
    assert written == pk.nbytes + sum(v.nbytes for v in keys.values()) == b.nbytes()
    r = CompressedEvaluationKeys.load(tmp_path / "bundle")
    assert r.header == b.header and r.key_ids() == b.key_ids() and r.mask_key == MASK
    assert np.array_equal(r.pk, pk) and isinstance(r.pk, np.memmap)
    for k, v in r.items():
        assert isinstance(v, np.memmap) and v.dtype == np.uint32 and np.array_equal(v, keys[k])
        assert np.array_equal(r[k], keys[k])


def test_streamed_bundle_saves_key_by_key(tmp_path):
    """as EvaluationKeys: an iterator of halves is consumed one at a time through ONE reused buffer"""
    from evaluation_keys import CompressedEvaluationKeys
    pk, keys = _halves(1)
    buf = np.zeros(max(v.size for v in keys.values()), np.uint32)
    live = []

    def produce():
        for k in sorted(keys):
            live.append(k)
            assert len(live) == 1  # the consumer took the previous key before asking for this one
            buf[:keys[k].size] = keys[k]
            yield k, buf[:keys[k].size]
            live.pop()

    b = CompressedEvaluationKeys(_header(), pk, produce())
    with pytest.raises(ValueError, match="streamed"):
        b.key_ids()
    b.save(tmp_path)
    r = CompressedEvaluationKeys.load(tmp_path)
    for k in keys:
        assert np.array_equal(r[k], keys[k])
    with pytest.raises(ValueError, match="consumed"):
        list(b.items())


def test_header_validation(tmp_path):
    from evaluation_keys import CompressedEvaluationKeys
    pk, keys = _halves(2)
    with pytest.raises(ValueError, match="version"):
        CompressedEvaluationKeys(dict(_header(), version=1), pk, keys)
    with pytest.raises(ValueError, match="version"):
        CompressedEvaluationKeys(dict(_header(), version=3), pk, keys)
    for bad in (MASK.hex()[:-1], MASK.hex() + "0", "g" * 64, MASK, 7, None):
        with pytest.raises(ValueError, match="64 hex digits"):
            CompressedEvaluationKeys(dict(_header(), mask_key=bad), pk, keys)
    no_mask = {k: v for k, v in _header().items() if k != "mask_key"}
    with pytest.raises(ValueError, match="mask_key"):
        CompressedEvaluationKeys(no_mask, pk, keys)
    with pytest.raises(ValueError, match="unknown header fields"):
        CompressedEvaluationKeys(dict(_header(), context_key="00" * 32), pk, keys)
    with pytest.raises(ValueError, match="moduli"):
        CompressedEvaluationKeys(dict(_header(), moduli=MODULI[:-1]), pk, keys)
    with pytest.raises(ValueError, match="duplicate"):
        list(CompressedEvaluationKeys(_header(), pk, iter([((0, -1), keys[(0, -1)]), ((0, -1), keys[(0, -1)])])).items())
    with pytest.raises(ValueError, match="low_p off"):
        CompressedEvaluationKeys(_header(low_p=False), pk, keys)
    # the public-key half is n_q << log_n words: neither one short nor the whole public key
    for wrong in (pk[:-1], np.concatenate([pk, pk])):
        with pytest.raises(ValueError, match="public key half"):
            CompressedEvaluationKeys(_header(), wrong, keys)
    with pytest.raises(ValueError, match="uint32"):
        CompressedEvaluationKeys(_header(), pk, {(0, -1): keys[(0, -1)].astype(np.int64)})
    # the same checks on what load reads
    CompressedEvaluationKeys(_header(), pk, keys).save(tmp_path)
    doc = json.loads((tmp_path / "header.json").read_text())
    for bad, match in ((dict(doc, header=dict(doc["header"], version=7)), "version"),
                       (dict(doc, header=dict(doc["header"], mask_key="xyz")), "64 hex digits"),
                       (dict(doc, keys=doc["keys"] + [doc["keys"][0]]), "duplicate"),
                       (dict(doc, header=dict(doc["header"], low_p=False)), "low_p off"),
                       (dict(doc, header=dict(doc["header"], secret=[1])), "unknown header fields")):
        (tmp_path / "header.json").write_text(json.dumps(bad))
        with pytest.raises(ValueError, match=match):
            CompressedEvaluationKeys.load(tmp_path)


def test_each_loader_refuses_the_other_format_and_load_bundle_dispatches(tmp_path):
    from evaluation_keys import CompressedEvaluationKeys, EvaluationKeys, load_bundle, make_header
    pk, keys = _halves(3)
    CompressedEvaluationKeys(_header(), pk, keys).save(tmp_path / "v2")
    full = {k: np.concatenate([v, v]) for k, v in keys.items()}
    EvaluationKeys(make_header(**_params()), np.concatenate([pk, pk]), full).save(tmp_path / "v1")
    with pytest.raises(ValueError, match="version 2"):
        EvaluationKeys.load(tmp_path / "v2")
    with pytest.raises(ValueError, match="version 1"):
        CompressedEvaluationKeys.load(tmp_path / "v1")
    with pytest.raises(ValueError, match="version"):           # and in memory: a v1 header is no v2 header
        CompressedEvaluationKeys(make_header(**_params()), pk, keys)
    v1, v2 = load_bundle(tmp_path / "v1"), load_bundle(tmp_path / "v2")
    assert type(v1) is EvaluationKeys and type(v2) is CompressedEvaluationKeys
    assert not isinstance(v2, EvaluationKeys) and v2.mask_key == MASK
    assert all(np.array_equal(v2[k], keys[k]) for k in keys) and all(np.array_equal(v1[k], full[k]) for k in keys)
    doc = json.loads((tmp_path / "v2" / "header.json").read_text())
    (tmp_path / "v2" / "header.json").write_text(json.dumps(dict(doc, header=dict(doc["header"], version=3))))
    with pytest.raises(ValueError, match="version 3"):
        load_bundle(tmp_path / "v2")


def test_file_names_and_nothing_named_for_a_secret_on_disk(tmp_path):
    """The mask key is public and named for what it is; `mask_key` itself contains the letters "sk", so it is taken
    out of a name before the search, as tests/test_evaluation_keys.py takes "ksk" out of the file names."""
    from evaluation_keys import COMPRESSED_HEADER_FIELDS, HEADER_FIELDS, CompressedEvaluationKeys
    pk, keys = _halves(4)
    CompressedEvaluationKeys(_header(), pk, keys).save(tmp_path)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == _file_names(keys)
    doc = json.loads((tmp_path / "header.json").read_text())
    assert set(doc) == {"header", "keys"}
    assert set(doc["header"]) == set(COMPRESSED_HEADER_FIELDS) == set(HEADER_FIELDS) | {"mask_key"}
    fields = set(doc) | set(doc["header"])
    for w in ("secret", "sparse", "sk"):
        assert not any(w in n.lower().replace("ksk", "") for n in names), w
        assert not any(w in f.lower().replace("mask_key", "") for f in fields), w
    # the 32 bytes of the mask key are in the header and in no key file
    assert doc["header"]["mask_key"] == MASK.hex()
    assert np.load(tmp_path / "pk_b.npy").nbytes == pk.nbytes
    for (g, l), v in keys.items():
        assert np.load(tmp_path / f"ksk_{g}_{'full' if l < 0 else l}_b.npy").nbytes == v.nbytes


def test_mask_prf_is_the_oracles_chacha():
    """tests/helpers/mask_prf.py against oracle.ckks_cpu.chacha_block (itself pinned to RFC 8439): 96 (key, counter,
    nonce) triples, counters and nonces above 2^32 among them, and the vectorised call against the one-at-a-time one"""
    from mask_prf import chacha_u64, key_words, stream_id, uniform_rows
    from oracle import ckks_cpu
    ckks_cpu.build()
    rng = np.random.default_rng(0xC4AC4A)
    keys = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(4)] + [bytes(32), bytes([255]) * 32]
    ctrs = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, (37 << 16) + 12345, 2 ** 63 + 5, 2 ** 64 - 1]
    ctrs += [int(x) for x in rng.integers(0, 2 ** 63, 8, dtype=np.uint64)]
    nonces = [stream_id(2), stream_id(4, 2 * 8192 - 1, 3), stream_id(10, 5, 2), stream_id(4, 2 ** 17 + 1, 0), 0, 2 ** 64 - 1]
    n = 0
    for key in keys:
        kw = key_words(key)
        assert kw.dtype == np.uint32 and int(kw[0]) == int.from_bytes(key[:4], "little")
        got = chacha_u64(key, np.array(nonces, np.uint64).reshape(-1, 1), np.array(ctrs, np.uint64).reshape(1, -1))
        assert got.shape == (len(nonces), len(ctrs)) and got.dtype == np.uint64
        for i, nonce in enumerate(nonces):
            for j, ctr in enumerate(ctrs):
                blk = ckks_cpu.chacha_block(kw, ctr, nonce)
                assert int(got[i, j]) == int(blk[0]) | (int(blk[1]) << 32), (key.hex(), ctr, nonce)
                n += 1
    assert n >= 64
    # uniform_rows: row i, coefficient k is prf(key, stream, (prime << log_n) + k) mod q of that prime
    rows = uniform_rows(keys[0], stream_id(4, 0, 1), [0, 3, 4], MODULI, LOG_N)
    assert rows.shape == (3, N) and rows.dtype == np.uint32
    for i, p in enumerate([0, 3, 4]):
        for k in (0, 1, N - 1):
            blk = ckks_cpu.chacha_block(key_words(keys[0]), (p << LOG_N) + k, stream_id(4, 0, 1))
            assert int(rows[i, k]) == (int(blk[0]) | (int(blk[1]) << 32)) % MODULI[p]
