"""The bench line's contract, checked on the committed line of the last profiled run (profiles/): every key the driver
and the judge read is there and self-consistent.  (bench.py itself needs a GPU; this keeps its output format honest.)"""
import glob
import json
import os

from conftest import ROOT


def _latest():
    """The newest committed DEFAULT line (`python bench.py --full`: C2 headline + CPU baseline + the other configs); round 1 committed
    only per-workload lines."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_bench_default.json"))) or sorted(glob.glob(os.path.join(ROOT, "profiles", "*_bench_C2.json")))
    assert files, "no committed bench line"
    return json.loads(open(files[-1]).read().strip().splitlines()[-1])


def test_bench_line_has_the_contract_keys():
    d = _latest()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["scaling"] == "strong"
    assert d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert "C2" in d["config"]["workload"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    if r["bound"] == "hbm":                                      # rounds 1-2: BASELINE's algorithmic-bytes model as the headline
        assert r["unit"] == "GB/s"
    else:                                                        # round 3 on: the bound that is real, f64 VALU issue; the model beside it
        assert r["bound"] == "f64_valu" and r["frac"] <= 1.0 and "model_hbm" in r
        m = r["model_hbm"]
        assert m["exceeds_hbm_peak"] == (m["achieved_GBps"] > m["peak_GBps"]) and abs(m["ratio"] - m["achieved_GBps"] / m["peak_GBps"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["cores"] >= 1


def test_bench_line_is_self_consistent():
    d = _latest()
    samples = 800 * 800 * 1024
    assert abs(d["value"] - samples / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    r = d["roofline"]
    if r["bound"] == "hbm":
        assert abs(r["achieved"] - r["bytes_per_sample"] * samples / (r["kernel_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
        alg = r["algorithmic_bytes_per_launch"]
    else:
        from raytracinginrust_amd import workloads
        assert r["ops_per_sample"] == workloads.valu_ops(workloads.F64_OPS_PER_SAMPLE["C2"])
        assert abs(r["achieved"] - r["ops_per_sample"] * r["samples_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e12) < 1e-6 * r["achieved"]
        assert r["peak"] == workloads.F64_VALU_PEAK_OPS / 1e12
        alg = r["model_hbm"]["algorithmic_bytes_per_launch"]
    assert r["kernel_ms"] <= d["ms_per_step"] * 1.001            # the kernel is inside the step
    if r["traffic"] is not None:                                 # only quoted from a PMC profile of the same kernel build
        assert r["framebuffer_atomic_bytes_per_launch"] < r["traffic"] < alg


def test_bench_line_times_the_other_configs():
    """Round 2 on: the default (`--full`) line carries C1, C3, C4 and C5 on the driver's clock, each with the committed bytes/sample."""
    from raytracinginrust_amd import workloads
    d = _latest()
    if "workloads" not in d:
        import pytest
        pytest.skip("the committed line predates the `workloads` block")
    assert set(d["workloads"]) == {"C1", "C3", "C4", "C5"}
    for key, e in d["workloads"].items():
        w = workloads.WORKLOADS[key]
        assert e["bytes_per_sample"] == workloads.BYTES_PER_SAMPLE[key]
        assert abs(e["value"] - w.samples / (e["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * e["value"] and e["steps"] >= 1
        assert e["kernel_ms"] <= e["ms_per_step"] * 1.001
        if d["roofline"]["bound"] == "hbm":
            assert abs(e["frac"] - e["bytes_per_sample"] * w.samples / (e["kernel_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
        else:
            ops = workloads.valu_ops(workloads.F64_OPS_PER_SAMPLE[key])
            assert e["ops_per_sample"] == ops and e["frac"] <= 1.0
            assert abs(e["frac"] - ops * w.samples / (e["kernel_ms"] * 1e-3) / workloads.F64_VALU_PEAK_OPS) < 1e-9
            assert abs(e["model_hbm_ratio"] - e["bytes_per_sample"] * w.samples / (e["kernel_ms"] * 1e-3) / 1e9 / 8000.0) < 1e-9
    c = d["cpu_baseline"]
    assert "reference_shaped" in c and c["reference_shaped"]["value"] > 0 and "flags" in c and "compiler" in c
    r = d["roofline"]
    assert (r["bytes_per_sample"] if r["bound"] == "hbm" else r["model_hbm"]["bytes_per_sample"]) == workloads.BYTES_PER_SAMPLE["C2"]


def test_bench_never_refuses_a_bare_gpus_flag():
    """`python bench.py --gpus N` must produce a line however the driver launches it: bare (this process drives the N GPUs), or under
    torch.distributed.run (one process per GPU; the launcher's world size wins over a stale --gpus)."""
    import importlib.util
    import pytest
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for n in (2, 4, 8):
        assert bench.resolve_mode("auto", n, 1) == (True, n)            # no launcher: in-process, rt_render_multi_device
        assert bench.resolve_mode("inproc", n, 1) == (True, n)
        assert bench.resolve_mode("auto", n, n) == (False, n)           # torch.distributed.run: one process per GPU
        assert bench.resolve_mode("procs", n, n) == (False, n)
        assert bench.resolve_mode("auto", 1, n) == (False, n)           # the launcher's world size is the number of GPUs
        with pytest.raises(ValueError, match="torch.distributed.run"):
            bench.resolve_mode("procs", n, 1)
    assert bench.resolve_mode("auto", 1, 1) == (False, 1)
    assert bench.resolve_mode("inproc", 1, 1) == (False, 1)
