"""bench.py through its driver-facing entry point on the GPU box: `--gpus N` really starts N ranks (two ranks share the
single GPU of the test box, so the process group is gloo there; RCCL is exercised with a one-rank group), the work queue is
broadcast and sharded, and the sharded job computes the same rows as a single rank."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + [str(a) for a in args], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_two_ranks_compute_the_same_rows_as_one(tmp_path):
    common = ("--steps", 2, "--warmup", 1, "--total-clips", 4, "--no-cpu-baseline", "--no-extra", "--lanes", 1)
    d2 = _bench("--gpus", 2, "--same-device", "--backend", "gloo", "--clips", 2, "--dump-out", tmp_path / "two.npy", *common)
    d1 = _bench("--gpus", 1, "--clips", 4, "--dump-out", tmp_path / "one.npy", *common)
    assert d2["n_gpus"] == 2 and d1["n_gpus"] == 1
    assert d2["config"]["work_queue"]["broadcast"] == "gloo" and d2["config"]["work_queue"]["clips_this_rank"] == 2
    assert d2["value"] > 0 and d2["roofline"]["frac"] > 0
    two, one = np.load(tmp_path / "two.npy"), np.load(tmp_path / "one.npy")
    assert two.shape == one.shape == (256, 2) and np.isfinite(one).all()
    # rank 0 holds clips 0, 2 and rank 1 clips 1, 3 (dist.shard: c mod world == rank); gathered rank-major
    order = [0, 2, 1, 3]
    for pos, clip in enumerate(order):
        np.testing.assert_array_equal(two[pos * 64:(pos + 1) * 64], one[clip * 64:(clip + 1) * 64])


def test_four_ranks_on_one_device_whole_job_with_a_ragged_tail(tmp_path):
    """The shape of the driver's multi-GPU run on the one GPU of the test box: 4 gloo ranks sharing cuda:0 on REAL compute (with the
    test process, no more than five processes hold the GPU), the whole 6-clip queue walked once (ranks 0-1 hold two clips, ranks 2-3
    one: their second step is NaN-padded), the clip pool generated once across the job and all-gathered, four per-rank rows.
    Gathered rows of the last step equal the single-rank run."""
    common = ("--whole-job", "--total-clips", 6, "--distinct-clips", 6, "--warmup", 1, "--no-cpu-baseline", "--no-extra", "--lanes", 1)
    d4 = _bench("--gpus", 4, "--same-device", "--backend", "gloo", "--clips", 1, "--dump-out", tmp_path / "four.npy", *common, timeout=1500)
    d1 = _bench("--gpus", 1, "--clips", 6, "--dump-out", tmp_path / "one.npy", *common)
    assert d4["n_gpus"] == 4 and d4["steps"] == 2 and d4["scaling"] == "strong" and d1["steps"] == 1
    pr = d4["per_rank"]
    assert [x["rank"] for x in pr] == list(range(4)) and all(x["device"] == 0 for x in pr)
    assert [x["frames"] for x in pr] == [128] * 2 + [64] * 2
    # 6 contents over 4 ranks: ceil = 2 per rank -> ranks 0-2 generate 2, rank 3 none; nothing twice
    assert [x["clip_contents_generated"] for x in pr] == [2, 2, 2, 0]
    assert all(x["startup_s"] > 0 and x["cpus"] >= 1 for x in pr)
    print("4 ranks on one device: startup %.1f-%.1f s, cpus per rank %s, bound %s" % (
        min(x["startup_s"] for x in pr), max(x["startup_s"] for x in pr), sorted({x["cpus"] for x in pr}), sorted({x["numa_node"] is not None for x in pr})))
    four, one = np.load(tmp_path / "four.npy"), np.load(tmp_path / "one.npy")
    assert four.shape == (4 * 64, 2) and one.shape == (6 * 64, 2) and np.isfinite(one).all()
    for r in range(4):                       # last step: rank r's second clip is clip 4 + r (c mod 4 == r), ranks 2-3 have none
        rows = four[r * 64:(r + 1) * 64]
        if r < 2:
            np.testing.assert_array_equal(rows, one[(4 + r) * 64:(5 + r) * 64])
        else:
            assert np.isnan(rows).all()


def test_dump_outputs_are_the_last_timed_step_and_repeat_bit_for_bit(tmp_path):
    """`--dump-outputs DIR` on real compute: the rows of the last timed step (the same rows `--dump-out` saves), and with the same
    arguments the same inputs and so the same bits in a second process."""
    common = ("--steps", 3, "--warmup", 1, "--clips", 4, "--total-clips", 8, "--distinct-clips", 8, "--no-cpu-baseline", "--no-extra")
    a = _bench("--dump-outputs", tmp_path / "a", "--dump-out", tmp_path / "rows.npy", *common)
    b = _bench("--dump-outputs", tmp_path / "b", *common)
    assert a["steps"] == b["steps"] == 3 and a["ms_per_step"] > 0
    va, vb = np.load(tmp_path / "a" / "valence_arousal.npy"), np.load(tmp_path / "b" / "valence_arousal.npy")
    assert va.dtype == np.float32 and va.shape == (4 * 64, 2) and np.isfinite(va).all()
    np.testing.assert_array_equal(va, np.load(tmp_path / "rows.npy"))
    np.testing.assert_array_equal(va, vb)


def test_one_rank_process_group_over_rccl():
    """The broadcast / all-gather / barrier / max-reduce path on RCCL itself (a one-rank group is all a 1-GPU box allows)."""
    d = _bench("--gpus", 1, "--force-dist", "--steps", 2, "--warmup", 1, "--clips", 2, "--no-cpu-baseline", "--no-extra")
    assert d["n_gpus"] == 1 and d["config"]["work_queue"]["broadcast"] == "nccl" and d["value"] > 0


def test_forced_process_group_agrees_with_the_plain_single_rank_run():
    """SCALE's N = 1 point must equal BENCH: the same step with and without the (one-rank, RCCL) process group -- identical
    rows, throughput within run-to-run noise -- and the forced run carries the per-rank diagnostic row."""
    common = ("--gpus", 1, "--steps", 8, "--warmup", 3, "--no-cpu-baseline", "--no-extra")     # the full 32-clip step
    a = _bench(*common)
    b = _bench("--force-dist", *common)
    assert "per_rank" not in a and len(b["per_rank"]) == 1 and b["per_rank"][0]["frames"] == 8 * 32 * 64
    assert b["per_rank"][0]["ms_per_step_local"] <= b["per_rank"][0]["ms_per_step"] * 1.001
    # Round 3 found the RCCL group costing 4 % here: its stream took the hardware queue of a lane.
    # Fresh processes of ONE mode differ by up to ~1 % (clocks, allocator state): each mode runs twice, interleaved, the better run
    # of each is compared, and the assert allows 2 %.
    a2 = _bench(*common)
    b2 = _bench("--force-dist", *common)
    ratio = max(b["value"], b2["value"]) / max(a["value"], a2["value"])
    print("force-dist / plain throughput: %.4f (runs: plain %.0f %.0f, forced %.0f %.0f)" % (ratio, a["value"], a2["value"], b["value"], b2["value"]))
    assert 0.98 < ratio < 1.02, ratio


def test_streamed_input_gives_the_same_rows_and_rate(tmp_path):
    """--stream-input: every step's uint8 frames come from pinned host memory through the copy stream.  Bit-identical rows;
    the default line's extra.streamed reports it beside the resident form."""
    common = ("--steps", 3, "--warmup", 1, "--clips", 6, "--total-clips", 12, "--distinct-clips", 12, "--no-cpu-baseline")
    a = _bench("--no-extra", "--dump-out", tmp_path / "res.npy", *common)
    b = _bench("--stream-input", "--extra-steps", 2, "--dump-out", tmp_path / "str.npy", *common)
    assert "streamed" in b["config"]["input"] and "streamed" not in a["config"]["input"]
    np.testing.assert_array_equal(np.load(tmp_path / "res.npy"), np.load(tmp_path / "str.npy"))
    st = b["extra"]["streamed"]
    assert st["pcie_bytes_per_step"] == 6 * 64 * 112 * 112 * 3 and st["value"] > 0 and st["resident_value"] > 0
    print("streamed / resident: %.4f (%.2f GB/s over PCIe)" % (st["streamed_over_resident"], st["pcie_GB_per_s"]))
    assert st["streamed_over_resident"] > 0.9


def test_default_line_has_the_contract_fields():
    d = _bench("--steps", 2, "--warmup", 1, "--clips", 4, "--cpu-clips", 1, "--extra-steps", 1)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert "uint8" in d["config"]["workload"] and d["dtype"] == "f32" and d["vs_baseline"] is None
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "step_floor_ms", "mixed_frac", "mixed"):
        assert k in d["roofline"], k
    # this run uses 4 clips per step: the committed PMC summaries are for the 32-clip step, so the PMC-derived fields are null
    # here (and say why); the default 32-clip line carries them (tests/test_host_logic.py checks that profiles/ has the files)
    assert d["roofline"]["mixed_frac"] is None and "note" in d["roofline"]["mixed"]
    ph = d["roofline_phase"]
    assert ph["floor_mfma_ms"] > ph["floor_hbm_ms"] > 0 and 0 < ph["frac_of_limiting_floor"] < 1
    # round 6: per-kernel floors of the phase stage (HBM, MFMA for the pyramid, VALU issue from the live SQ pass) and their sum; the sustained
    # clock of the conv launches and the fraction of the MFMA peak at that clock beside the nominal one (null with a reason when the
    # profiler is not on the box)
    ks = ph["kernels"]
    assert set(ks) == {"pyramid_frame", "phase_window2<48>", "phase_window2<24>"}
    assert ks["pyramid_frame"]["limiter"] == "mfma" and all(k["floor_ms"] > 0 and 0 < k["frac_of_floor"] < 1 for k in ks.values())
    assert abs(ph["limiting_floor_ms"] - sum(k["floor_ms"] for k in ks.values())) < 1e-9 and "pyramid_frame:mfma" in ph["limiting_floor"]
    r = d["roofline"]
    for k in ("sustained_clock_GHz", "mfma_busy_frac", "peak_at_sustained_clock", "frac_at_sustained_clock", "clock_note"):
        assert k in r, k
    if r["sustained_clock_GHz"] is not None:
        assert 1.2 <= r["sustained_clock_GHz"] <= 2.4 * 1.03 and 0 < r["mfma_busy_frac"] < 1 and r["frac_at_sustained_clock"] >= r["frac"] * 0.97
        assert ks["phase_window2<48>"]["limiter"] == "valu" and ph["floor_valu_ms"] > 0
    else:
        assert "no live SQ" in r["clock_note"]
    assert d["hot_path_steps_executed"] >= 5
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["cpu_model"] and cb["deduplicated"]["value"] > 0
    # round 5: what the CPU figure is made of (library versions, per-stage rates) and the "as tuned" variant beside the reference-faithful one
    assert "MKL" in cb["torch_cpu_libraries"] or "OpenMP" in cb["torch_cpu_libraries"]
    assert cb["stage_rates"]["resnet50_GFLOP_per_s_per_process"] > 0 and cb["as_tuned"]["value"] > 0
    assert cb["as_tuned"]["stage_rates"]["resnet50_GFLOP_per_s_per_process"] > 0
    ex = d["extra"]
    assert ex["direct_form"]["value"] > 0 and ex["multi_snippet"]["gru_seq_len"] == 5 and ex["multi_snippet"]["value"] > 0
    assert ex["streamed"]["value"] > 0 and ex["streamed"]["pcie_GB_per_s"] > 0
    assert ex["bf16x3"]["value"] > 0 and ex["bf16x3"]["max_abs_diff_vs_fp32_outputs"] < 1e-4 and ex["bf16x3"]["layers"]["launches"] > 10
    # round 5: per-stage rates for BASELINE configs[1] / configs[2] in the driver-visible line
    for k in ("clips_32", "clips_256"):
        assert ex["phase_only"][k]["value"] > 1e5 and 0 < ex["phase_only"][k]["frac_of_hbm_peak"] < 1
    for k in ("batch_64", "batch_256"):
        assert ex["resnet50_only"][k]["value"] > 1e3 and 0 < ex["resnet50_only"][k]["frac_of_fp32_mfma_peak_algorithmic"] < 1.2
    assert d["parity_vs_cpu_sample"]["max_abs_err_valence_arousal"] < 1e-4
