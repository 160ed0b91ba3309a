"""bench.py's stdout line stays parseable by the driver (VERDICT r4 'do this' 1): the full record
of round 4's final bench (profiles/r4_bench_final.json, 83 KB, every leg with per-class rooflines)
goes through the same compact_line / emit_line the bench prints with, and must come out as ONE
JSON line under 12 KB that keeps every contract key and each leg's number."""
import json
import sys

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

FULL = ROOT / "profiles" / "r4_bench_final.json"


def _full():
    return json.loads(FULL.read_text())


def test_line_under_limit_and_round_trips(tmp_path):
    full = _full()
    assert len(json.dumps(full)) > 60_000  # the record that did not parse
    detail = tmp_path / "detail.json"
    s = bench.emit_line(full, str(detail))
    assert "\n" not in s
    assert len(s) < 12_000
    line = json.loads(s)
    assert json.loads(detail.read_text()) == full  # nothing lost: the detail file holds the whole record
    assert line["detail_file"] == str(detail)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "roofline_step", "cpu_baseline"):
        assert k in line, k
    assert line["config"]["workload"].startswith("C2")
    assert abs(line["value"] - full["value"]) / full["value"] < 1e-5
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r
    assert abs(r["frac"] - full["roofline"]["frac"]) < 1e-4
    cb = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb
    for leg in ("batch", "batch_pairs", "batch_packed_pairs", "true_fhe", "eager_ref_calls"):
        assert leg in line and line[leg]["roofline_step"]["frac"] > 0
    assert line["batch"]["roundtrip"]["roundtrip_blocks_per_s"] > 0
    # per-class entries are numeric arrays in the documented field order
    cls = line["roofline_step"]["classes"]["ntt_rows_fwd"]
    assert len(cls) == len(bench.CLASS_FIELDS) and all(isinstance(x, (int, float)) or x is None for x in cls)
    # the prose appears once, in notes
    assert s.count("dispatch-inclusive duration") == 1
    assert line["roofline_step"]["traffic_over_algorithmic"]["ntt_rows_fwd"] > 0.5


def test_line_without_detail_file_and_oversize_fallback():
    full = _full()
    s = bench.emit_line(full, None)
    assert len(s) < 12_000 and "detail_file" not in json.loads(s)
    # a record with many more legs still fits: the per-class arrays of secondary legs are dropped first
    for i in range(6):
        full[f"extra_{i}"] = full["batch"]
    saved = bench.LEG_KEYS
    try:
        bench.LEG_KEYS = saved + tuple(f"extra_{i}" for i in range(6))
        s = bench.emit_line(full, None)
    finally:
        bench.LEG_KEYS = saved
    assert len(s) < 12_000
    json.loads(s)


def test_sig_rounding():
    assert bench._sig(0.362346652, 3) == 0.362
    assert bench._sig(47095808.0, 4) == 47100000.0
    assert bench._sig(5) == 5 and bench._sig(None) is None and bench._sig(True) is True


def test_plain_run_is_the_default_and_full_keeps_the_detail_file(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.detail_json == "" and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.detail_json.endswith("bench_detail.json") and a.dump_outputs == "d"


def test_plain_record_gives_a_line_with_the_contract_keys():
    """a plain run's record: no roofline, precision, leg or baseline, verification not done (None)"""
    full = {k: v for k, v in _full().items() if k not in bench.LEG_KEYS + ("cpu_baseline",)}
    full.update(roofline=None, roofline_secondary=None, roofline_valu=None, roofline_step=None, precision=None,
                dumped_outputs={"bytes": [16]})
    full["config"]["verified_against_plaintext_model"] = None
    line = json.loads(bench.emit_line(full, None))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert line[k] is not None, k
    assert line["roofline"] is None and line["dumped_outputs"] == {"bytes": [16]} and "cpu_baseline" not in line


def test_dump_outputs_files(tmp_path, monkeypatch):
    """--dump-outputs: float arrays per ciphertext and the decoded bytes; an array over its share of the
    size limit is written as the same seeded sample every time"""
    import numpy as np

    class Eng:
        def export(self, ct):
            return np.arange(2 * 3 * 64, dtype=np.uint32).reshape(2, 3, 64) + ct

    class Ctx:
        engine = Eng()

        def decrypt(self, ct):
            return np.exp(2j * np.pi * (np.arange(32) + ct) / 16)

    class Pipe:
        class encoder:
            @staticmethod
            def decode(hi, lo):
                return np.arange(16, dtype=np.uint8)

    shapes = bench.dump_outputs(tmp_path / "a", Pipe, Ctx(), (1, 2))
    got = {p.name: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["bytes.npy", "ct_hi_residues.npy", "ct_hi_slots.npy", "ct_lo_residues.npy", "ct_lo_slots.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["ct_lo_residues.npy"], Eng().export(2)) and shapes["ct_hi_slots"] == [2, 32]
    assert np.array_equal(got["bytes.npy"], np.arange(16))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 5 * 800)  # 100 float64 per array: the residues (384) are sampled
    bench.dump_outputs(tmp_path / "b", Pipe, Ctx(), (1, 2))
    bench.dump_outputs(tmp_path / "c", Pipe, Ctx(), (1, 2))
    b, c = np.load(tmp_path / "b" / "ct_hi_residues.npy"), np.load(tmp_path / "c" / "ct_hi_residues.npy")
    assert b.shape == (100,) and np.array_equal(b, c) and np.isin(b, got["ct_hi_residues.npy"]).all()
    assert sum(p.stat().st_size for p in (tmp_path / "b").iterdir()) <= 5 * 800 + 5 * 128
