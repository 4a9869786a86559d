"""bench.py --gpus N must launch N ranks by itself (--gpus was never read)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env,
                          timeout=300)


def test_gpus_2_spawns_two_ranks_dry_run():
    r = _run(["--gpus", "2", "--dry-run", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout                     # ONE JSON line, from rank 0
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["dry_run"] is True


def test_config3_dry_run_shards_the_volume_over_two_ranks():
    """bench.py --workload config3 --gpus 2 --dry-run (gloo): the sharded bench path of BASELINE configs[2] - disjoint contiguous slice shares in rank
    order, barrier, MAX over ranks - before hardware sees it."""
    r = _run(["--gpus", "2", "--dry-run", "--workload", "config3", "--slices", "4", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["dry_run"] is True and rec["unit"] == "slices/s"
    assert rec["config"]["slice_seeds_per_rank"] == [[3000, 3001, 3002, 3003], [3004, 3005, 3006, 3007]]


def test_world_size_mismatch_fails_loudly():
    r = _run(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_too_few_gpus_fails_loudly():
    # no GPU in the CPU container: asking for 2 GPUs without --dry-run must refuse instead of running 1 rank
    import torch
    if torch.cuda.device_count() >= 2:
        return
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"])
    assert r.returncode != 0 and "GPU(s) visible" in (r.stderr + r.stdout)


def test_roofline_traffic_is_reported_only_for_the_code_it_was_measured_on(monkeypatch):
    """bench.pmc_traffic: the committed PMC table counts only while the kernel sources hash to the value stored with it - a table of
    other code is named and refused (round 2 shipped a round-1 constant)."""
    import json

    import bench
    tables = sorted(n for n in os.listdir(os.path.join(ROOT, "profiles")) if n.endswith("_pmc_traffic.json"))
    assert tables
    newest = json.load(open(os.path.join(ROOT, "profiles", tables[-1])))
    sha = newest["_meta"]["csrc_sha16"]
    monkeypatch.setattr(bench, "csrc_sha16", lambda: sha)
    value, source = bench.pmc_traffic("up_fused_kernel<1, 1>")
    assert value == newest["up_fused_kernel"]["hbm_bytes_per_launch"] and value > 1e9 and sha in source
    monkeypatch.setattr(bench, "csrc_sha16", lambda: "0" * 16)
    value, source = bench.pmc_traffic("up_fused_kernel<1, 1>")
    assert value is None and "other code" in source and sha in source
    value, source = bench.pmc_traffic("no_such_kernel")
    assert value is None and "no PMC table" in source
    # the hash names the sources: it moves with any byte of csrc/ or the ABI header
    monkeypatch.undo()
    assert len(bench.csrc_sha16()) == 16 and bench.csrc_sha16() == bench.csrc_sha16()


def test_final_line_is_compact_strict_json_and_carries_the_judged_fields():
    """round 5's 24 KB line overflowed the driver's 8000-character stdout tail (BENCH_r05.parsed == null).  The final line is
    built by bench.compact_line: < 6 KB, strict JSON (no NaN / Infinity tokens), with roofline + cpu_baseline + every parity leg inside."""
    import bench

    def strict_loads(text):
        def refuse(tok):
            raise ValueError(f"non-standard JSON token {tok}")
        return json.loads(text, parse_constant=refuse)

    canned = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line.json")))        # the very line that failed to parse
    assert len(json.dumps(canned)) > 20000
    # poison it: NaN / inf anywhere in the tree must come out as null, numpy scalars as numbers
    import numpy as np
    canned["mask_iou_vs_ref"]["min"] = float("nan")
    canned["roofline"]["traffic"] = float("inf")
    canned["interactive_side"]["predict_ms_median"] = np.float32(0.85)
    canned["mask_iou_vs_ref_split16"] = dict(canned["mask_iou_vs_ref_strict"])
    canned["mask_iou_vs_ref_trained"]["split16"] = dict(canned["mask_iou_vs_ref_trained"]["strict"])
    text = bench.compact_line(canned, "gpurun_out/bench_extras.json")
    assert "\n" not in text and len(text) < bench.LINE_LIMIT == 6144, len(text)
    rec = strict_loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in rec, k
    assert rec["value"] == canned["value"] and rec["config"]["workload"].startswith("configs[1]")
    roof = rec["roofline"]
    assert roof["bound"] == "mfma" and roof["frac"] == canned["roofline"]["frac"] and roof["traffic"] is None and "whole_path_frac" in roof
    assert "other_kernels" not in roof and "pipes" not in roof
    assert set(rec["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"}
    for leg in ("mask_iou_vs_ref", "mask_iou_vs_ref_strict", "mask_iou_vs_ref_split16"):
        assert set(rec[leg]) >= {"n_instances", "frac_ge_0.999", "min", "keep_set", "identical_id_frac_foreground"}, leg
        assert "worst" not in rec[leg]
    assert rec["mask_iou_vs_ref"]["min"] is None                                            # the poisoned NaN
    assert rec["mask_iou_vs_ref_strict"]["tiles_per_s"] == canned["mask_iou_vs_ref_strict"]["tiles_per_s"]
    trained = rec["mask_iou_vs_ref_trained"]
    assert set(trained) == {"default", "split16", "strict"} and trained["default"]["frac_ge_0.999"] < 0.9 < trained["strict"]["frac_ge_0.999"]
    assert rec["train_side"]["vit_b"]["non_hip_device_time_frac"] == canned["train_side"]["vit_b"]["non_hip_device_time_frac"]
    # a tree that would still be too long sheds optional blocks instead of overflowing
    canned["config"]["workload"] = "w" * 3000
    canned["dtype"] = "d" * 2500
    text = bench.compact_line(canned, "gpurun_out/bench_extras.json")
    assert len(text) < bench.LINE_LIMIT
    rec = strict_loads(text)
    assert rec["roofline"]["frac"] == canned["roofline"]["frac"] and rec["cpu_baseline"]["value"] == canned["cpu_baseline"]["value"]


def test_emit_prints_the_full_tree_before_the_final_line(tmp_path, monkeypatch, capsys):
    import bench
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    canned = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line.json")))
    bench.emit(canned)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and lines[0].startswith("bench_extras: {") and lines[1].startswith("{") and len(lines[1]) < bench.LINE_LIMIT
    assert len(lines[0]) > 20000
    full = json.load(open(tmp_path / "gpurun_out" / "bench_extras.json"))
    assert "other_kernels" in full["roofline"] and "worst" in full["mask_iou_vs_ref"]
    assert json.loads(lines[1])["extras"] == os.path.join("gpurun_out", "bench_extras.json")


def test_steps_below_one_is_refused():
    r = _run(["--steps", "0", "--dry-run"])
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_writes_seeded_float_arrays_under_the_limit(tmp_path):
    """bench.py --dump-outputs DIR: the same seeded sample of an output in every run, float32 / float64 .npy files, 64 MiB in all at most."""
    import numpy as np
    import pytest

    import bench
    pick = bench.dump_sample(64, 8)
    assert len(pick) == 8 and list(pick) == sorted(set(pick.tolist())) and pick.max() < 64
    assert np.array_equal(pick, bench.dump_sample(64, 8)) and len(bench.dump_sample(3, 8)) == 3
    arrays = {"labels": np.arange(12, dtype=np.float32).reshape(3, 4), "tile_seeds": np.arange(3, dtype=np.float64) + 1000}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["labels.npy", "tile_seeds.npy"]
    for name, a in arrays.items():
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype == a.dtype and np.array_equal(a, b)
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "e"), {"labels": np.zeros(4, np.int32)})
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "f"), {"labels": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
    assert not (tmp_path / "f").exists()


def test_plain_run_line_carries_the_contract_fields_without_the_full_run_blocks():
    """A plain run (no --full) prints compact_line of the contract fields + config: strict JSON, no extras path, no parity or side blocks;
    --full is accepted next to the other options."""
    import bench
    canned = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_line.json")))
    contract = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    plain = {k: canned[k] for k in contract}
    plain["config"] = {k: canned["config"][k] for k in ("workload", "tiles_per_step_per_gpu", "encoder_batch", "decode_lanes")}
    plain["roofline"] = None
    rec = json.loads(bench.compact_line(plain))
    assert all(rec[k] == plain[k] for k in contract) and rec["config"] == plain["config"]
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and "extras" not in rec
    assert not [k for k in rec if k.startswith(("mask_iou", "pcie", "api_", "train_", "config3", "split16", "fp8", "interactive"))]
    r = _run(["--dry-run", "--full", "--steps", "1", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
