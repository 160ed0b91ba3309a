"""EvaluationKeys -- what a client hands a server so that it can evaluate without the secret.

A bundle is a small header (format version, the parameter set and its moduli), the public key and the switching
keys as ``(galois tag, level) -> flat uint32 array`` (level -1: a full key, level >= 0: that reduced level's own
key).  It never holds the secret key, the sparse secret of the bootstrap, or the client's PRNG key or seed: the
header has no field for them and ``save`` writes none.

On disk: ``header.json`` plus one ``.npy`` per key (``pk.npy``, ``ksk_<tag>_<level>.npy`` with ``full`` for level
-1).  ``load`` memory-maps the arrays, and both ``save`` and ``EngineContext.from_evaluation_keys`` accept the
keys as a lazily produced iterator, so a bundle of several GB is never held in host memory at once.

``CompressedEvaluationKeys`` (format version 2) is the same bundle at half the size: a client built
with a public mask key ships the ``b`` half of every key and the mask key in the header, and the server regenerates
the ``a`` halves on its device.  ``load_bundle`` reads whichever of the two a directory holds.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Iterable, Iterator, Tuple

import numpy as np

FORMAT_VERSION = 1
HEADER_FIELDS = ("version", "log_n", "max_level", "dnum", "bootstrappable", "low_p", "n_q", "n_p", "moduli")
_HEADER_FILE = "header.json"
_PK_FILE = "pk.npy"

KeyId = Tuple[int, int]


def _key_file(galois: int, level: int) -> str:
    return f"ksk_{int(galois)}_{'full' if level < 0 else int(level)}.npy"


def make_header(*, log_n: int, max_level: int, dnum: int, bootstrappable: bool, low_p: bool, n_q: int, n_p: int, moduli) -> dict:
    """the header of a bundle: `max_level` is the engine's constructor level (the fresh level of a bootstrappable
    set), `moduli` its n_q + n_p primes in the engine's order (Q chain, then the special primes)"""
    h = dict(version=FORMAT_VERSION, log_n=int(log_n), max_level=int(max_level), dnum=int(dnum), bootstrappable=bool(bootstrappable),
             low_p=bool(low_p), n_q=int(n_q), n_p=int(n_p), moduli=[int(m) for m in np.asarray(moduli).ravel()])
    validate_header(h)
    return h


def validate_header(h: dict) -> None:
    if not isinstance(h, dict):
        raise ValueError("evaluation keys: the header is not a mapping")
    if h.get("version") != FORMAT_VERSION:
        raise ValueError(f"evaluation keys: format version {h.get('version')!r}, this reader knows version {FORMAT_VERSION}")
    extra = set(h) - set(HEADER_FIELDS)
    if extra:
        raise ValueError(f"evaluation keys: unknown header fields {sorted(extra)}")
    missing = [f for f in HEADER_FIELDS if f not in h]
    if missing:
        raise ValueError(f"evaluation keys: header fields missing: {missing}")
    if len(h["moduli"]) != h["n_q"] + h["n_p"]:
        raise ValueError(f"evaluation keys: {len(h['moduli'])} moduli for n_q + n_p = {h['n_q']} + {h['n_p']}")
    if not all(1 < int(m) < 2 ** 32 for m in h["moduli"]):
        raise ValueError("evaluation keys: a modulus outside (1, 2^32)")


def _check_id(header: dict, kid: KeyId, seen: set) -> KeyId:
    g, level = int(kid[0]), int(kid[1])
    if g < 0 or level < -1:
        raise ValueError(f"evaluation keys: bad key id {kid!r}")
    if (g, level) in seen:
        raise ValueError(f"evaluation keys: duplicate key id (galois {g}, level {level})")
    if level >= 0 and not header["low_p"]:
        raise ValueError(f"evaluation keys: a reduced-level key (galois {g}, level {level}) in a bundle whose header says low_p off")
    seen.add((g, level))
    return g, level


def _flat_u32(a) -> np.ndarray:
    a = np.asanyarray(a)  # a memory-mapped array stays one
    if a.dtype != np.uint32:
        raise ValueError(f"evaluation keys: key arrays are uint32, not {a.dtype}")
    return a.reshape(-1)


class EvaluationKeys:
    """header + public key + switching keys.  `keys`: a mapping ``(galois, level) -> array`` or an iterable of
    ``((galois, level), array)`` pairs; a mapping is validated at once, an iterable as it is consumed (`items`)."""

    def __init__(self, header: dict, pk, keys):
        validate_header(header)
        self.header = dict(header)
        self.pk = _flat_u32(pk)
        want = 2 * self.header["n_q"] << self.header["log_n"]
        if self.pk.size != want:
            raise ValueError(f"evaluation keys: the public key has {self.pk.size} words, this parameter set's has {want}")
        if isinstance(keys, dict):
            seen: set = set()
            self._keys = {_check_id(self.header, k, seen): _flat_u32(v) for k, v in keys.items()}
            self._stream = None
        else:
            self._keys = None
            self._stream = iter(keys)

    def key_ids(self) -> list:
        if self._keys is None:
            raise ValueError("evaluation keys: a streamed bundle has no key list before it is consumed")
        return sorted(self._keys)

    def __getitem__(self, kid: KeyId) -> np.ndarray:
        if self._keys is None:
            raise ValueError("evaluation keys: a streamed bundle is read through items()")
        return self._keys[(int(kid[0]), int(kid[1]))]

    def items(self) -> Iterator[Tuple[KeyId, np.ndarray]]:
        """((galois, level), flat uint32 array) of every key, validated; a streamed bundle can be read once"""
        if self._keys is not None:
            for k in sorted(self._keys):
                yield k, self._keys[k]
            return
        stream, self._stream = self._stream, None
        if stream is None:
            raise ValueError("evaluation keys: this streamed bundle was already consumed")
        seen: set = set()
        for kid, arr in stream:
            yield _check_id(self.header, kid, seen), _flat_u32(arr)

    def nbytes(self) -> int:
        """bytes of the public key and every held key (a streamed bundle: the public key alone)"""
        return int(self.pk.nbytes + sum(v.nbytes for v in (self._keys or {}).values()))

    # ------------------------------------------------------------------ disk
    def save(self, directory) -> int:
        """writes header.json, pk.npy and one .npy per key, key by key as items() produces them; returns the bytes of
        key material written"""
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        np.save(d / _PK_FILE, self.pk)
        total, ids = int(self.pk.nbytes), []
        for (g, level), arr in self.items():
            np.save(d / _key_file(g, level), arr)
            ids.append([g, level])
            total += int(arr.nbytes)
        (d / _HEADER_FILE).write_text(json.dumps({"header": self.header, "keys": ids}, indent=1))
        return total

    @classmethod
    def load(cls, directory) -> "EvaluationKeys":
        """the bundle `save` wrote, its arrays memory-mapped (read as they are imported, never all at once)"""
        d = Path(directory)
        doc = json.loads((d / _HEADER_FILE).read_text())
        if not isinstance(doc, dict) or set(doc) != {"header", "keys"}:
            raise ValueError("evaluation keys: header.json holds a header and a key list, nothing else")
        header = doc["header"]
        validate_header(header)
        seen: set = set()
        ids = [_check_id(header, k, seen) for k in doc["keys"]]
        pk = np.load(d / _PK_FILE, mmap_mode="r", allow_pickle=False)
        keys = {k: np.load(d / _key_file(*k), mmap_mode="r", allow_pickle=False) for k in ids}
        return cls(header, pk, keys)


# ---------------------------------------------------------------------- seed-compressed bundles
COMPRESSED_FORMAT_VERSION = 2
COMPRESSED_HEADER_FIELDS = HEADER_FIELDS + ("mask_key",)
_PK_HALF_FILE = "pk_b.npy"


def _key_half_file(galois: int, level: int) -> str:
    return f"ksk_{int(galois)}_{'full' if level < 0 else int(level)}_b.npy"


def make_compressed_header(*, mask_key, **params) -> dict:
    """the version-2 header: make_header's fields plus the public mask key (32 bytes, or its 64 hex digits)"""
    h = dict(make_header(**params), version=COMPRESSED_FORMAT_VERSION,
             mask_key=mask_key.hex() if isinstance(mask_key, (bytes, bytearray)) else mask_key)
    validate_compressed_header(h)
    return h


def validate_compressed_header(h: dict) -> None:
    if not isinstance(h, dict):
        raise ValueError("compressed evaluation keys: the header is not a mapping")
    if h.get("version") != COMPRESSED_FORMAT_VERSION:
        raise ValueError(f"compressed evaluation keys: format version {h.get('version')!r}, this reader knows version "
                         f"{COMPRESSED_FORMAT_VERSION} (version {FORMAT_VERSION} is EvaluationKeys')")
    extra = set(h) - set(COMPRESSED_HEADER_FIELDS)
    if extra:
        raise ValueError(f"compressed evaluation keys: unknown header fields {sorted(extra)}")
    if "mask_key" not in h:
        raise ValueError("compressed evaluation keys: header fields missing: ['mask_key']")
    mk = h["mask_key"]
    if not isinstance(mk, str) or len(mk) != 64 or any(c not in "0123456789abcdefABCDEF" for c in mk):
        raise ValueError("compressed evaluation keys: mask_key is not 64 hex digits")
    validate_header({**{k: v for k, v in h.items() if k != "mask_key"}, "version": FORMAT_VERSION})  # the shared fields


class CompressedEvaluationKeys:
    """EvaluationKeys' interface over the b halves: `pk` is [n_q][N], a key [dnum][nkey][N] (full), [nkey][N] (the
    dense -> sparse key, a reduced level's key) or [2][nkey][N] (a ring key, tag 12 N + ring, DESIGN.md §3.29: the key
    `EngineContext.ensure_ring_key` adds), each half the words of its EvaluationKeys counterpart; the header
    carries the public mask key the a halves are regenerated from.  Never the secret, nor the client's own key."""

    def __init__(self, header: dict, pk, keys):
        validate_compressed_header(header)
        self.header = dict(header)
        self.pk = _flat_u32(pk)
        want = self.header["n_q"] << self.header["log_n"]
        if self.pk.size != want:
            raise ValueError(f"compressed evaluation keys: the public key half has {self.pk.size} words, this parameter set's has {want}")
        if isinstance(keys, dict):
            seen: set = set()
            self._keys = {_check_id(self.header, k, seen): _flat_u32(v) for k, v in keys.items()}
            self._stream = None
        else:
            self._keys = None
            self._stream = iter(keys)

    # the key list, the lookup, the validated (streamed) iteration and the byte count are EvaluationKeys' own
    key_ids = EvaluationKeys.key_ids
    __getitem__ = EvaluationKeys.__getitem__
    items = EvaluationKeys.items
    nbytes = EvaluationKeys.nbytes

    @property
    def mask_key(self) -> bytes:
        return bytes.fromhex(self.header["mask_key"])

    def save(self, directory) -> int:
        """writes header.json, pk_b.npy and one ksk_<tag>_<level|full>_b.npy per key, key by key as items() produces
        them; returns the bytes of key material written (the mask key lives in the header)"""
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        np.save(d / _PK_HALF_FILE, self.pk)
        total, ids = int(self.pk.nbytes), []
        for (g, level), arr in self.items():
            np.save(d / _key_half_file(g, level), arr)
            ids.append([g, level])
            total += int(arr.nbytes)
        (d / _HEADER_FILE).write_text(json.dumps({"header": self.header, "keys": ids}, indent=1))
        return total

    @classmethod
    def load(cls, directory) -> "CompressedEvaluationKeys":
        """the bundle `save` wrote, its arrays memory-mapped"""
        d = Path(directory)
        doc = json.loads((d / _HEADER_FILE).read_text())
        if not isinstance(doc, dict) or set(doc) != {"header", "keys"}:
            raise ValueError("compressed evaluation keys: header.json holds a header and a key list, nothing else")
        header = doc["header"]
        validate_compressed_header(header)
        seen: set = set()
        ids = [_check_id(header, k, seen) for k in doc["keys"]]
        pk = np.load(d / _PK_HALF_FILE, mmap_mode="r", allow_pickle=False)
        keys = {k: np.load(d / _key_half_file(*k), mmap_mode="r", allow_pickle=False) for k in ids}
        return cls(header, pk, keys)


def load_bundle(directory):
    """EvaluationKeys or CompressedEvaluationKeys, as the format version in the directory's header.json selects"""
    doc = json.loads((Path(directory) / _HEADER_FILE).read_text())
    version = doc.get("header", {}).get("version") if isinstance(doc, dict) and isinstance(doc.get("header"), dict) else None
    if version == FORMAT_VERSION:
        return EvaluationKeys.load(directory)
    if version == COMPRESSED_FORMAT_VERSION:
        return CompressedEvaluationKeys.load(directory)
    raise ValueError(f"evaluation keys: format version {version!r}, this reader knows versions {FORMAT_VERSION} and {COMPRESSED_FORMAT_VERSION}")


def stream_keys(engine, ids: Iterable[KeyId] | None = None) -> Iterator[Tuple[KeyId, np.ndarray]]:
    """((galois, level), array) of the engine's present keys (or `ids`), read out one at a time into ONE reused host
    buffer: each array is valid until the next is produced (save and from_evaluation_keys consume them in step)"""
    ids = list(engine.key_ids() if ids is None else ids)
    if not ids:
        return
    buf = np.empty(max(engine.ksk_words(g, lv) for g, lv in ids), np.uint32)
    for g, lv in ids:
        yield (g, lv), engine.export_key(g, lv, out=buf)


def stream_key_halves(engine, ids: Iterable[KeyId] | None = None) -> Iterator[Tuple[KeyId, np.ndarray]]:
    """stream_keys for the b halves (Engine.export_key_half): one reused host buffer of half the size"""
    ids = list(engine.key_ids() if ids is None else ids)
    if not ids:
        return
    buf = np.empty(max(engine.ksk_words(g, lv) for g, lv in ids) // 2, np.uint32)
    for g, lv in ids:
        yield (g, lv), engine.export_key_half(g, lv, out=buf)
