"""Host-side logic of the product package (no GPU): snippet/window index plan, result assembly,
multi-process sharding + gather over gloo (world_size 2), deterministic generators."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

from mimamo_net_amd import sampler, weights, synthetic, dist as mdist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_snippet_ranges_and_window_ids_match_reference(golden):
    g = golden("sampler")
    for n in (10, 64, 100, 128, 309):
        r = sampler.snippet_ranges(n, 64, 64)
        np.testing.assert_array_equal(np.array(r), g["ranges_%d" % n])
        ids = np.stack([sampler.window_ids(s, e, n) for s, e in r])
        assert ids.dtype == np.int32
        np.testing.assert_array_equal(ids % 251, g["ids_%d" % n])
    with pytest.raises(ValueError):
        sampler.snippet_ranges(0)
    assert sampler.snippet_ranges(1) == [[0, 1]]
    np.testing.assert_array_equal(sampler.window_ids(0, 1, 1), np.zeros((1, 13), dtype=np.int32))


def test_product_sampler_equals_oracle(oracle):
    for n in (1, 5, 63, 64, 65, 127, 200, 1000):
        assert sampler.snippet_ranges(n) == oracle.snippet_ranges(n)
        for s, e in sampler.snippet_ranges(n):
            np.testing.assert_array_equal(sampler.window_ids(s, e, n), oracle.window_ids(s, e, n))


def test_assemble_overwrite_order_and_coverage():
    r = sampler.snippet_ranges(150)
    assert r == [[0, 64], [64, 128], [86, 150]]
    preds = [np.full((64, 2), k + 1.0) for k in range(3)]
    v = sampler.assemble(preds, r)
    assert v.shape == (150, 2) and v.dtype == np.float64
    assert (v[:64] == 1).all() and (v[64:86] == 2).all() and (v[86:] == 3).all()
    # like the reference (api/tester.py:112-118, min_f starts at 0) an uncovered prefix is NOT detected:
    v2 = sampler.assemble(preds[1:], r[1:])
    assert (v2[:64] == 0).all()


def test_generators_are_deterministic_and_layouts_complete():
    a = weights.det_uniform("x", (7, 3), -1, 1, 5)
    b = weights.det_uniform("x", (7, 3), -1, 1, 5)
    np.testing.assert_array_equal(a, b)
    assert abs(float(weights.det_uniform("y", (100000,), -1, 1, 1).mean())) < 0.01
    sd = weights.make_two_stream_state_dict(1)
    assert len(sd) == 107 and sum(v.size for k, v in sd.items() if v.dtype == np.float32) == 2636425 + sum(
        sd[k + s].size for k in weights.TWO_STREAM_BN_KEYS for s in (".running_mean", ".running_var"))
    assert weights.two_stream_blob(sd).size == 2640783
    rs = weights.make_resnet50_state_dict(1)
    assert len(weights.resnet50_layers()) == 53 and weights.resnet50_blob(rs).size == 23561152
    c1, c2 = synthetic.make_clip_u8(3, 4), synthetic.make_clip_u8(3, 4)
    np.testing.assert_array_equal(c1, c2)
    assert c1.std() > 10  # textured, never constant


def test_shard_policies():
    assert mdist.shard(10, 0, 4) == [0, 4, 8] and mdist.shard(10, 3, 4) == [3, 7]
    lengths = [300, 64, 64, 64, 200, 100]
    parts = [mdist.shard(6, r, 2, lengths) for r in range(2)]
    assert sorted(parts[0] + parts[1]) == list(range(6))
    loads = [sum(lengths[i] for i in p) for p in parts]
    assert abs(loads[0] - loads[1]) <= 100


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    import mimamo_net_amd  # noqa: F401
    from mimamo_net_amd import dist as md
    r, w, _ = md.init("gloo")
    lengths = [64, 100, 37, 64, 128]

    def compute(idx):  # stand-in for the per-video hot path: rows depend only on (video, frame)
        rows = [np.stack([np.full(lengths[i], i, dtype=np.float32), np.arange(lengths[i], dtype=np.float32)], 1) for i in idx]
        return torch.from_numpy(np.concatenate(rows)) if rows else torch.zeros((0, 2))

    res = md.run_sharded(lengths, compute, r, w)
    ok = all(res[i].shape == (lengths[i], 2) and (res[i][:, 0] == i).all() and (res[i][:, 1] == np.arange(lengths[i])).all()
             for i in range(len(lengths)))
    q.put((rank, ok, sorted(res)))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_two_process_gloo_shard_and_gather():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in got) and all(keys == [0, 1, 2, 3, 4] for _, _, keys in got)


# ---- bench.py launcher / work queue (the driver-facing multi-GPU entry point), with a stub compute on CPU ranks --------
def _run_bench(*args, env=None, timeout=240):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ if env is None else env)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        if env is None:
            e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + [str(a) for a in args], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus_flag_spawns_that_many_ranks(tmp_path):
    """`bench.py --gpus 2` without a torchrun environment starts two ranks itself (gloo here), broadcasts the work queue
    from rank 0, shards it round-robin and all-gathers the rows: one JSON line with n_gpus == 2."""
    dump = str(tmp_path / "rows.npy")
    r, d = _run_bench("--gpus", 2, "--stub-compute", "--steps", 3, "--warmup", 1, "--clips", 2, "--total-clips", 10,
                      "--distinct-clips", 10, "--dump-out", dump)
    assert r.returncode == 0, r.stderr[-2000:]
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["value"] > 0
    q = d["config"]["work_queue"]
    assert q["total_clips"] == 10 and q["clips_this_rank"] == 5 and q["broadcast"] == "gloo"
    rows = np.load(dump)                       # last step (index 3 incl. warm-up): rank 0 holds clips 0,2,4,6,8; rank 1 the odd ones
    assert rows.shape == (2 * 2 * 64, 2)
    # step s takes shard positions 2s, 2s+1 (wrapping): s = 3 -> positions 6,7 -> 1,2 -> clips 2,4 (rank 0), 3,5 (rank 1)
    assert list(rows[::64, 0]) == [2, 4, 3, 5] and (rows[:64, 1] == np.arange(64)).all()


def test_bench_eight_ranks_report_one_row_per_rank():
    """The driver's scaling run ends at 8 ranks: same launcher path with 8 stub ranks (gloo), and the JSON line carries one
    diagnostic row per rank (its own step time, the step time incl. the wait for peers, its frames, the queue broadcast time)
    so that a poor 8-GPU number can be attributed to a rank, to the gather or to the communicator set-up."""
    r, d = _run_bench("--gpus", 8, "--stub-compute", "--steps", 2, "--warmup", 1, "--clips", 2, "--total-clips", 64,
                      "--distinct-clips", 64, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert d["n_gpus"] == 8 and d["config"]["work_queue"]["clips_this_rank"] == 8
    pr = d["per_rank"]
    assert [x["rank"] for x in pr] == list(range(8))
    assert all(x["frames"] == 2 * 2 * 64 for x in pr)
    assert all(x["ms_per_step"] >= x["ms_per_step_local"] >= 0 and x["queue_broadcast_ms"] >= 0 for x in pr)
    assert abs(max(x["ms_per_step"] for x in pr) - d["ms_per_step"]) < 1e-6          # the headline time IS the slowest rank's
    assert d["value"] == pytest.approx(8 * 2 * 2 * 64 / (d["ms_per_step"] * 2 * 1e-3), rel=1e-6)
    # round 4: every rank reports where its start-up time went and which CPUs it was pinned to (no NUMA information without a
    # GPU: the allowed CPUs are split evenly; disjoint slices, together no more than the host has)
    ncpu = len(os.sched_getaffinity(0))
    assert all(x["startup_s"] >= x["process_group_init_s"] >= 0 and x["weights_s"] >= 0 for x in pr)
    assert all(x["cpus"] >= 1 and x["numa_node"] is None for x in pr)
    if ncpu >= 8:
        firsts = [x["first_cpu"] for x in pr]
        assert len(set(firsts)) == 8 and sum(x["cpus"] for x in pr) == ncpu, (firsts, ncpu)


def test_bind_rank_cpus_splits_the_allowed_cpus(tmp_path):
    """dist.bind_rank_cpus in a child process (it changes the caller's affinity): even, disjoint, covering slices of the allowed
    CPUs when the platform has no NUMA information; a single rank stays unbound."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, os, json; sys.path.insert(0, %r); import mimamo_net_amd; from mimamo_net_amd import dist; "
            "a = sorted(os.sched_getaffinity(0)); r, w = int(sys.argv[1]), int(sys.argv[2]); i = dist.bind_rank_cpus(r, w); "
            "print(json.dumps({'info': i, 'before': a, 'after': sorted(os.sched_getaffinity(0))}))" % root)
    outs = [json.loads(subprocess.run([sys.executable, "-c", code, str(r), "3"], stdout=subprocess.PIPE, universal_newlines=True,
                                      check=True).stdout.splitlines()[-1]) for r in range(3)]
    allowed = outs[0]["before"]
    if len(allowed) >= 3:
        got = [o["after"] for o in outs]
        assert sorted(c for g in got for c in g) == allowed and all(o["info"]["bound"] and o["info"]["cpus"] == len(o["after"]) for o in outs)
    one = json.loads(subprocess.run([sys.executable, "-c", code, "0", "1"], stdout=subprocess.PIPE, universal_newlines=True,
                                    check=True).stdout.splitlines()[-1])
    assert one["after"] == one["before"] and not one["info"]["bound"]
    from mimamo_net_amd import dist
    assert dist._parse_cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]


def test_bench_gpus_flag_must_match_launcher_world_size():
    r, d = _run_bench("--gpus", 4, "--stub-compute", env=dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert r.returncode != 0 and d is None and "does not match WORLD_SIZE" in r.stderr


def test_bench_dump_outputs_writes_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR`: the rows the last of the `--steps` timed steps returned, float32, as DIR/valence_arousal.npy."""
    out = tmp_path / "out"
    r, d = _run_bench("--stub-compute", "--steps", 3, "--warmup", 1, "--clips", 2, "--total-clips", 10, "--distinct-clips", 10,
                      "--dump-outputs", out)
    assert r.returncode == 0, r.stderr[-2000:]
    assert d["steps"] == 3 and d["ms_per_step"] >= 0
    assert sorted(os.listdir(out)) == ["valence_arousal.npy"]
    rows = np.load(out / "valence_arousal.npy")
    # one warm-up + 3 timed steps of 2 clips: the last takes queue positions 6, 7
    assert rows.dtype == np.float32 and rows.shape == (2 * 64, 2) and list(rows[::64, 0]) == [6, 7]
    r, d = _run_bench("--stub-compute", "--steps", 0, "--dump-outputs", out)
    assert r.returncode != 0 and d is None and "--steps" in r.stderr


def test_bench_dump_outputs_samples_rows_over_the_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 16 * 100)
    rows = np.arange(1000 * 2, dtype=np.float32).reshape(1000, 2)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), rows)
    got, idx = np.load(tmp_path / "a" / "valence_arousal.npy"), np.load(tmp_path / "a" / "valence_arousal_rows.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64 and got.shape == (100, 2) and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(got, rows[idx.astype(np.int64)])
    np.testing.assert_array_equal(got, np.load(tmp_path / "b" / "valence_arousal.npy"))      # the same sample every time
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_LIMIT_BYTES


def test_bench_whole_job_walks_the_queue_once_with_a_ragged_tail(tmp_path):
    dump = str(tmp_path / "rows.npy")
    r, d = _run_bench("--gpus", 3, "--stub-compute", "--whole-job", "--total-clips", 11, "--clips", 2, "--distinct-clips", 11,
                      "--dump-out", dump)
    assert r.returncode == 0, r.stderr[-2000:]
    assert d["n_gpus"] == 3 and d["steps"] == 2 and d["scaling"] == "strong"
    rows = np.load(dump)[::64, 0]              # last step: rank 0 -> 6, 9; rank 1 -> 7, 10; rank 2 -> 8 and one empty slot
    assert list(rows[:5]) == [6, 9, 7, 10, 8] and np.isnan(rows[5])


def test_bench_refuses_to_run_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU host")
    r, d = _run_bench("--steps", 1, "--no-cpu-baseline")
    assert r.returncode != 0 and d is None and "no CPU path" in r.stderr


def test_bench_under_torchrun_as_the_driver_launches_it():
    """`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2`: ranks come from the launcher's environment,
    rank 0 prints the one JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--clips", "2", "--stub-compute"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["config"]["work_queue"]["total_clips"] == 10000


# ---- drop-in Dataset classes (Snippet_Sampler / Image_Sampler by name), pinned by the fixtures frozen from the real classes ----------
def _video_tree(d, n, side, value_of=None, clip=None):
    from PIL import Image
    feat, root = os.path.join(d, "feat"), os.path.join(d, "v_opface")
    os.makedirs(feat)
    os.makedirs(os.path.join(root, "v_aligned"))
    for i in range(1, n + 1):
        np.save(os.path.join(feat, "%05d.npy" % i), np.full((4,), i, dtype=np.float32))
        img = clip[i - 1] if clip is not None else np.full((side, side, 3), value_of(i), dtype=np.uint8)
        Image.fromarray(img, "RGB").save(os.path.join(root, "v_aligned", "frame_det_00_%06d.bmp" % i))
    return root, feat


def test_snippet_sampler_dataset_matches_the_real_class(golden, tmp_path):
    """mimamo_net_amd.Snippet_Sampler on the directory trees tests/golden/make_golden.py built for the real class (G7, G12): same
    seq_ranges, same clamped windows (constant frames encode their index), same PIL-preprocessed planes; the uint8 mode hands
    the unique frames + window ids that reproduce the same windows."""
    import mimamo_net_amd
    from mimamo_net_amd import Snippet_Sampler
    g7, g12 = golden("sampler"), golden("sampler_keywords")
    cases = [(n, 64, 64, 12, "%d" % n, g7, 16) for n in (10, 100, 309)] + \
            [(int(n), int(l), int(s), int(p), "%d_%d_%d_%d" % (n, l, s, p), g12, 8) for n, l, s, p in g12["cases"] if n <= 100]
    for k, (n, length, stride, num_phase, tag, g, side) in enumerate(cases):
        d = str(tmp_path / ("v%d" % k))
        os.makedirs(d)
        root, feat = _video_tree(d, n, side, value_of=lambda i: (i - 1) % 251)
        ds = Snippet_Sampler("v", root, feat, annot_dir=None, label_name="valence_arousal", test_mode=True, num_phase=num_phase,
                             phase_size=8, length=length, stride=stride)
        np.testing.assert_array_equal(np.array(ds.seq_ranges), g["ranges_" + tag])
        du = Snippet_Sampler("v", root, feat, label_name="valence_arousal", num_phase=num_phase, phase_size=8, length=length,
                             stride=stride, return_u8=True)
        for j in range(len(ds)):
            ph, feats, lab, rng, name = ds[j]
            assert name == "v" and tuple(ph.shape) == (rng[1] - rng[0], num_phase + 1, 8, 8) and lab.shape == (rng[1] - rng[0], 2)
            assert (lab == -100).all() and np.array_equal(feats[:, 0].astype(np.int64) - 1, np.arange(rng[0], rng[1]))
            np.testing.assert_array_equal(np.rint(ph[:, :, 0, 0].numpy() * 255).astype(np.int64), g["ids_" + tag][j])
            u8, ids, feats2, _, rng2, _ = du[j]
            assert u8.dtype.is_floating_point is False and u8.shape[1:] == (side, side, 3) and list(rng2) == list(rng)
            np.testing.assert_array_equal(u8.numpy()[ids][:, :, 0, 0, 0].astype(np.int64), g["ids_" + tag][j])
            assert len(np.unique(ids)) == u8.shape[0]            # every frame of the snippet's windows decoded once
    # the preprocessing itself: textured 112x112 frames -> convert('L') + Lanczos 48 + /255, bit-equal to the real sampler
    from mimamo_net_amd import synthetic
    d = str(tmp_path / "tex")
    os.makedirs(d)
    root, feat = _video_tree(d, 3, 112, clip=synthetic.make_clip_u8(5, 3))
    ph = Snippet_Sampler("v", root, feat, label_name="valence_arousal")[0][0].numpy()
    np.testing.assert_array_equal(np.stack([ph[0, 6], ph[1, 6], ph[2, 6]]), g7["gray48_clip5"])
    with pytest.raises(NotImplementedError):
        Snippet_Sampler("v", root, feat, test_mode=False)
    with pytest.raises(ValueError):
        Snippet_Sampler("v", root, str(tmp_path / "nowhere"))


def test_image_sampler_dataset(tmp_path):
    from mimamo_net_amd import Image_Sampler, synthetic, sampler
    clip = synthetic.make_clip_u8(7, 4)
    d = str(tmp_path / "img")
    os.makedirs(d)
    root, _ = _video_tree(d, 4, 112, clip=clip)
    ds = Image_Sampler("v", root, test_mode=True, return_u8=True)
    assert len(ds) == 4
    for i in range(4):
        img, label, path, name = ds[i]
        assert name == "v" and path.endswith("frame_det_00_%06d.bmp" % (i + 1)) and list(label) == [-100]
        np.testing.assert_array_equal(img.numpy(), clip[i])
    # with the extractor's transform (api/resnet50_extractor.py:41,53): same tensors as the host loader of Resnet50_Extractor.run
    paths = [p for _, p in sampler.list_aligned_frames(root, "v")]
    want = sampler.load_rgb_batch(paths).numpy()

    def model_transform(im):      # Resize(256) + CenterCrop(224) + ToTensor + x255 + Normalize(mean, 1)  (utils/model_utils.py:26-40)
        import torch
        from PIL import Image
        im = im.convert('RGB').resize((256, 256), Image.BILINEAR).crop((16, 16, 240, 240))
        a = np.asarray(im, dtype=np.float32) / np.float32(255)
        return torch.from_numpy(a.transpose(2, 0, 1) * np.float32(255.0) - np.asarray(sampler.RESNET50_MEAN, dtype=np.float32)[:, None, None])

    dt = Image_Sampler("v", root, test_mode=True, transform=model_transform)
    np.testing.assert_array_equal(np.stack([dt[i][0].numpy() for i in range(4)]), want)
    default = Image_Sampler("v", root, test_mode=True, size=112)[0][0]
    assert tuple(default.shape) == (3, 112, 112) and abs(float(default.mean())) < 3.0
    with pytest.raises(NotImplementedError):
        Image_Sampler("v", root)                 # the reference's default is test_mode=False: training-time sampling


def test_profiles_hold_pmc_summaries_for_the_head_kernel_sources():
    """bench.py quotes roofline.traffic / roofline_phase.traffic / roofline.mixed_frac from PMC summaries under profiles/ and only
    while their `kernel_source_hash` equals the hash of mimamo-net_amd/csrc at HEAD: a kernel edit without a profile refresh would
    silently null those fields in the driver's line (round-3 verdict, weak item 9).  This test is the reminder."""
    import glob
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    head = bench.kernel_source_hash()
    found = {}
    for kind in ("conv_traffic", "phase_traffic", "layer_bytes"):
        for path in glob.glob(os.path.join(root, "profiles", "*%s*.json" % kind)):
            d = json.load(open(path))
            if d.get("kernel_source_hash") == head and d.get("clips_per_gpu") == 32:
                found[kind] = (os.path.basename(path), d)
    assert set(found) == {"conv_traffic", "phase_traffic", "layer_bytes"}, (
        "profiles/ has no PMC summary for kernel-source hash %s: re-run tools/profile_round.sh on the GPU box and copy "
        "gpurun_out/r0N_{conv,phase}_traffic_32clips.json + r0N_layer_bytes_32clips.json to profiles/ (found: %s)" % (head, sorted(found)))
    assert found["conv_traffic"][1]["bytes_per_step"] > 1e11 and found["phase_traffic"][1]["bytes_per_step"] > 5e8
    lb = found["layer_bytes"][1]
    assert len(lb["launches"]) > 90 and 0.5 < lb["mixed_frac"] < 1.0 and lb["step_floor_ms"] > 60


def test_live_traffic_leg_never_raises_without_a_profiler(monkeypatch):
    """bench.py measures roofline.traffic live by running itself under rocprofv3 --pmc (round 5); a box without the profiler -- or any failure
    of it -- must leave the bench line intact: the helper returns an error record and the committed PMC summary is quoted instead."""
    import shutil
    import sys
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    monkeypatch.setattr(shutil, "which", lambda name: None)
    real_exists = os.path.exists
    monkeypatch.setattr(os.path, "exists", lambda p: False if str(p).endswith("rocprofv3") else real_exists(p))
    out = bench.measure_live_traffic(types.SimpleNamespace(lanes=3), 32)
    assert out == {"error": "rocprofv3 not found"}


def _bench():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    return bench


def test_live_traffic_leg_survives_a_hung_profiler(monkeypatch, tmp_path):
    """Round-5 verdict item 5: with a `rocprofv3` that never returns, the default bench run must still print its line in time.  The live
    leg runs every profiler child in its own process group under a per-child timeout, kills the GROUP (the profiler forks the python
    child) and gives up after the first timeout instead of trying the remaining passes."""
    import shutil
    import subprocess
    import time
    import types
    bench = _bench()
    fake = tmp_path / "rocprofv3"
    pidfile = tmp_path / "grandchild.pid"
    # a profiler that forks a grandchild and hangs: both must be gone after the timeout
    fake.write_text("#!/bin/bash\nsleep 600 &\necho $! > %s\nsleep 600\n" % pidfile)
    fake.chmod(0o755)
    monkeypatch.setattr(shutil, "which", lambda name: str(fake))
    monkeypatch.setattr(bench, "LIVE_CHILD_TIMEOUT_S", 2)
    monkeypatch.setattr(bench, "LIVE_BUDGET_S", 30)
    args = types.SimpleNamespace(lanes=3, winograd=1, no_winograd=False, from_f32=False, stream_input=False)
    t0 = time.time()
    out = bench.measure_live_traffic(args, 32)
    assert time.time() - t0 < 15, "one child timeout, not one per pass"
    assert "error" in out and "no result after 2 s" in out["error"], out
    gpid = int(pidfile.read_text())
    time.sleep(0.2)
    alive = subprocess.run(["ps", "-o", "stat=", "-p", str(gpid)], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip()
    assert alive == "" or alive.startswith("Z"), "the profiler's grandchild survived the timeout: %r" % alive


def test_live_traffic_child_runs_the_parents_schedule():
    """the profiler child must launch the kernels its parent launches (flags that change the schedule are forwarded)."""
    import types
    bench = _bench()
    a = types.SimpleNamespace(lanes=2, winograd=4, no_winograd=True, from_f32=True, stream_input=False)
    f = bench.schedule_flags(a)
    assert f == ["--lanes", "2", "--winograd", "4", "--no-winograd", "--from-f32"]
    bench.parse_args(["--steps", "1"] + f)           # every forwarded flag is one bench.py accepts


def test_sq_pass_summary_and_phase_floors(tmp_path):
    """Round-5 verdict item 4: the line carries the sustained clock of the conv launches (GRBM_GUI_ACTIVE / kernel time), the fraction
    of the MFMA peak at that clock, and per-kernel floors of the phase stage incl. the VALU-issue floor (SQ_INSTS_VALU x 4 cycles /
    1 024 SIMDs / 2.4 GHz) -- the verdict's own example: 8.88e7 instructions -> 0.144 ms for phase_window2_kernel<48>."""
    bench = _bench()
    cc = tmp_path / "cc.csv"
    tr = tmp_path / "kt.csv"
    rows = [("void mm::conv_mfma_kernel<128,256>(p)", "GRBM_GUI_ACTIVE", 8 * 2.0e6), ("void mm::conv_mfma_kernel<128,256>(p)", "SQ_VALU_MFMA_BUSY_CYCLES", 0.9 * 1024 * 2.0e6),
            ("void mm::wino_fused_kernel<3,2>(p)", "GRBM_GUI_ACTIVE", 8 * 1.0e6), ("void mm::wino_fused_kernel<3,2>(p)", "SQ_VALU_MFMA_BUSY_CYCLES", 0.6 * 1024 * 1.0e6),
            ("void mm::phase_window2_kernel<48>(a)", "SQ_INSTS_VALU", 2 * 8.88e7), ("void mm::phase_window2_kernel<48>(a)", "SQ_INSTS_MFMA", 0.0),
            ("void mm::phase_window2_kernel<24>(a)", "SQ_INSTS_VALU", 2 * 2.4e7),
            ("void mm::pw::pyramid_wave_kernel<8>(a)", "SQ_INSTS_VALU", 2 * 4.0e7), ("void mm::pw::pyramid_wave_kernel<8>(a)", "SQ_INSTS_MFMA", 2 * 8.0e6),
            ("void mm::pf::pyramid_frame_kernel(a)", "SQ_INSTS_VALU", 2 * 1.0e7), ("void mm::pf::pyramid_frame_kernel(a)", "SQ_INSTS_MFMA", 2 * 0.9e6),
            ("void mm::wino_in6_kernel(a)", "GRBM_GUI_ACTIVE", 1e9)]
    cc.write_text("Kernel_Name,Counter_Name,Counter_Value\n" + "".join('"%s",%s,%r\n' % r for r in rows))
    tr.write_text("Kernel_Name,Start_Timestamp,End_Timestamp\n"
                  '"void mm::conv_mfma_kernel<128,256>(p)",1000,1001000\n"void mm::wino_fused_kernel<3,2>(p)",2000000,2500000\n"void mm::wino_in6_kernel(a)",0,5\n')
    # (the per-frame stage: pyramid_wave_kernel for whole rounds of 2 048 frames + pyramid_frame_kernel for a small remainder, one tag)
    pk = {"pyramid_frame": ("pyramid_wave_kernel", "pyramid_frame_kernel"), "phase_window2<48>": "phase_window2_kernel<48", "phase_window2<24>": "phase_window2_kernel<24"}
    clock, valu = bench.sq_pass_summary(str(cc), str(tr), 2, ("conv_mfma_kernel", "wino_fused_kernel"), pk)
    assert abs(clock["GHz"] - 3.0e6 / 1.5e6) < 1e-9                      # 3.0e6 cycles in 1.5 ms = 2.0 GHz
    assert abs(clock["mfma_busy"] - (0.9 * 2 + 0.6 * 1) / 3) < 1e-9
    assert valu == {"pyramid_frame": 5.0e7 - 8.9e6, "phase_window2<48>": 8.88e7, "phase_window2<24>": 2.4e7}
    live = [(0, 1e12, 9.0, "M=1 K=2 N=3"), (1, 2048 * 9216.0, 0.317, "pyramid_frame"), (2, 2048 * 221184.0, 0.40, "phase_window2<48>"),
            (2, 2048 * 55296.0, 0.11, "phase_window2<24>")]
    kern, total = bench.phase_floors(live, 2048, valu)
    assert abs(kern["phase_window2<48>"]["floor_valu_ms"] - 0.1445) < 1e-3 and kern["phase_window2<48>"]["limiter"] == "valu"
    assert kern["pyramid_frame"]["limiter"] == "mfma" and abs(kern["pyramid_frame"]["floor_mfma_ms"] - 0.1158) < 1e-3
    assert abs(total - sum(k["floor_ms"] for k in kern.values())) < 1e-12 and total > 0.116 + 0.144
    # without the SQ pass the floors fall back to HBM / MFMA and say so
    kern2, total2 = bench.phase_floors(live, 2048, None)
    assert "floor_valu_ms" not in kern2["phase_window2<48>"] and kern2["phase_window2<48>"]["limiter"] == "hbm" and total2 < total


def test_implausible_sustained_clock_is_dropped_not_reported():
    """A live profiler pass whose GRBM_GUI_ACTIVE and kernel trace disagree (seen on one box in round 6: 2.98 GHz on a 2.4 GHz part, the
    matrix-pipe busy fraction low by the same factor) must not put a `frac_at_sustained_clock` on the line."""
    bench = _bench()
    ok = {"GHz": 2.31, "mfma_busy": 0.77, "how": "x"}
    assert bench.plausible_clock(ok) == (ok, None)
    assert bench.plausible_clock(None) == (None, None)
    for bad in (2.975, 0.4, None):
        clk, note = bench.plausible_clock({"GHz": bad, "mfma_busy": 0.6, "how": "x"})
        assert clk is None and "rejected" in note


def test_every_profile_file_the_docs_quote_exists():
    """DESIGN.md / README.md / INTEGRATION.md and the profiles / tools indexes back their numbers with files under profiles/ (same-box A/B
    logs, rocprof summaries): a renamed or dropped log must not leave a dangling citation behind."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    missing = []
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md", os.path.join("profiles", "README.md"), os.path.join("tools", "README.md")):
        text = open(os.path.join(root, doc)).read()
        for m in re.finditer(r"(r0[1-9]_[A-Za-z0-9_.{},|*]+?\.(?:txt|json|csv|md))", text):
            name = m.group(1)
            if any(c in name for c in "{}*|,"):
                continue                       # a pattern (r04_{conv,phase}_traffic_...), not a file name
            if not os.path.exists(os.path.join(root, "profiles", name)):
                missing.append((doc, name))
    assert not missing, missing


MODEL_DEF = """
import torch
import torch.nn as nn


class Resnet50_ferplus_dag(nn.Module):

    def __init__(self):
        super(Resnet50_ferplus_dag, self).__init__()
        self.meta = {'mean': [%(mean)s],
                     'std': [1, 1, 1],
                     'imageSize': [224, 224, 3]}
        self.conv1_7x7_s2 = nn.Conv2d(3, 64, kernel_size=[7, 7], stride=(2, 2), padding=(3, 3), bias=False)
        self.conv1_7x7_s2_bn = nn.BatchNorm2d(64, eps=%(eps)s, momentum=0.1, affine=True, track_running_stats=True)
        self.conv1_relu_7x7_s2 = nn.ReLU()
        self.pool1_3x3_s2 = nn.MaxPool2d(kernel_size=[3, 3], stride=[2, 2], padding=(0, 0), dilation=1, ceil_mode=%(ceil)s)
        self.conv3_1_1x1_reduce = nn.Conv2d(256, 128, kernel_size=[1, 1], stride=(%(s1)d, %(s1)d), bias=False)
        self.conv3_1_3x3 = nn.Conv2d(128, 128, kernel_size=[3, 3], stride=(%(s3)d, %(s3)d), padding=(1, 1), bias=False)
        raise RuntimeError("a definition file is read, never executed")


def resnet50_ferplus_dag(weights_path=None, **kwargs):
    raise RuntimeError("a definition file is read, never executed")
"""


def test_model_definition_file_is_read_without_executing_it(tmp_path):
    """`<benchmark_dir>/ferplus/<model_name>.py` is the file the reference executes (api/utils/model_utils.py:65-79) to get the graph and
    `model.meta` (api/resnet50_extractor.py:38-41); the product reads the same facts with `ast`."""
    p = tmp_path / "resnet50_ferplus_dag.py"
    p.write_text(MODEL_DEF % dict(mean="131.0912, 103.8827, 91.4953", eps="1e-05", ceil="True", s1=2, s3=1))
    d = weights.read_model_definition(str(p))
    assert d == {"meta": {"mean": [131.0912, 103.8827, 91.4953], "std": [1, 1, 1], "imageSize": [224, 224, 3]},
                 "stride_on_first_1x1": True, "ceil_mode": True, "bn_eps": 1e-5}
    p.write_text(MODEL_DEF % dict(mean="91.5, 103.9, 131.1", eps="0.001", ceil="False", s1=1, s3=2))
    d = weights.read_model_definition(str(p))
    assert d["meta"]["mean"] == [91.5, 103.9, 131.1] and d["stride_on_first_1x1"] is False and d["ceil_mode"] is False
    assert d["bn_eps"] == 1e-3
    p.write_text("x = 1\n")
    assert weights.read_model_definition(str(p)) == {}


def test_conv_bias_is_folded_into_the_batchnorm_mean(oracle):
    """A checkpoint with conv biases (the published definition has bias=False; a re-export may not): BN(conv + b) == BN' (conv) with
    running_mean' = mean - b.  Checked on the blob and, through the oracle, on the first layer's output."""
    sd = weights.make_resnet50_state_dict(seed=3)
    plain = weights.resnet50_blob(sd)
    biased = dict(sd)
    for name, _, cout, _, _, _ in weights.resnet50_layers():
        biased[name + ".bias"] = weights.det_uniform(name + ".bias", (cout,), -0.5, 0.5, 3)
    blob = weights.resnet50_blob(biased)
    assert blob.shape == plain.shape and not np.array_equal(blob, plain)
    # first layer: conv weight 64*3*49, then gamma, beta, mean, var
    off = 64 * 3 * 49
    np.testing.assert_array_equal(blob[:off + 128], plain[:off + 128])
    np.testing.assert_allclose(blob[off + 128:off + 192], sd["conv1_7x7_s2_bn.running_mean"] - biased["conv1_7x7_s2.bias"], rtol=0, atol=1e-7)
    np.testing.assert_array_equal(blob[off + 192:off + 256], plain[off + 192:off + 256])
    folded = dict(sd)
    for name, _, _, _, _, _ in weights.resnet50_layers():
        folded[name + "_bn.running_mean"] = (sd[name + "_bn.running_mean"].astype(np.float64) - biased[name + ".bias"]).astype(np.float32)
    np.testing.assert_array_equal(weights.resnet50_blob(folded), blob)
