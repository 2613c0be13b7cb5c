"""bench.py's bookkeeping that needs no GPU: the committed counter summaries it prices the rooflines with (profiles/rNN_pmc_*.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_counter_summaries_are_found_and_template_instances_are_added_up(tmp_path, monkeypatch):
    import bench
    # the newest committed summary of every workload exists and names the kernels the rooflines ask for
    for workload, kernel in (("refine", "k_global"), ("refine", "k_local"), ("reconstruct", "k_insert_bricks"), ("sva", "k_sva_eval"), ("csp", "k_csp_eval")):
        name = bench.pmc_latest(workload)
        assert name and os.path.exists(os.path.join(ROOT, "profiles", name)), workload
        e, meta = bench.pmc_entry(name, kernel, merge=True)
        assert e and meta.get("particles"), (workload, kernel)
        assert e["SQ_INSTS_VALU"]["sum"] > 0 and "FETCH_SIZE" in e and "WRITE_SIZE" in e, (workload, kernel)
    # two instances of one kernel template: their counters are sums, per_dispatch follows
    d = {"_meta": {"particles": 4}, "ppm::k_x<0>": {"C": {"sum": 10.0, "dispatches": 2, "per_dispatch": 5.0}},
         "ppm::k_x<6>": {"C": {"sum": 30.0, "dispatches": 3, "per_dispatch": 10.0}}}
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    (tmp_path / "profiles").mkdir()
    json.dump(d, open(tmp_path / "profiles" / "t.json", "w"))
    e, _ = bench.pmc_entry("t.json", "k_x", merge=True)
    assert e["C"] == {"sum": 40.0, "dispatches": 5, "per_dispatch": 8.0}
    e, _ = bench.pmc_entry("t.json", "k_x<6>")
    assert e["C"]["sum"] == 30.0


def test_plain_run_times_the_headline_alone_and_full_keeps_every_block():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    assert a.no_cpu and a.no_side and a.no_dropin and a.no_next_rows
    f = bench.parse(["--full"])
    assert f.full and not (f.no_cpu or f.no_side or f.no_dropin or f.no_next_rows)
    f = bench.parse(["--full", "--no-cpu", "--dump-outputs", "d"])
    assert f.no_cpu and not f.no_side and f.dump_outputs == "d"


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import bench
    rows = np.arange(64.0).reshape(16, 4)
    bench.dump_outputs(str(tmp_path / "a"), {"rows": rows, "img": np.ones((3, 2), np.float16), "n": np.array([5, 7])})
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("rows", "img", "n")}
    assert got["rows"].dtype == np.float64 and np.array_equal(got["rows"], rows)
    assert got["img"].dtype == np.float32 and got["n"].dtype == np.float64 and list(got["n"]) == [5.0, 7.0]
    # beyond the budget: the same seeded rows of every array, in order, twice alike
    monkeypatch.setattr(bench, "DUMP_BYTES", (16 * 4 + 16) * 8 // 4)          # a quarter of what the two arrays hold
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"rows": rows, "idx": np.arange(16.0)})
    b, i = np.load(tmp_path / "b" / "rows.npy"), np.load(tmp_path / "b" / "idx.npy")
    assert b.shape == (4, 4) and np.array_equal(b, rows[i.astype(int)]) and np.all(np.diff(i) > 0)
    assert np.array_equal(b, np.load(tmp_path / "c" / "rows.npy"))
