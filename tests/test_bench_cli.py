"""bench.py's --gpus contract (the driver runs ``bench.py --gpus N`` with or
without torch.distributed.run): a world size that disagrees with --gpus, or
more ranks than visible GPUs, fails fast with a non-zero exit instead of
timing one GPU and reporting it as N."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    env.pop("PILOSA_BENCH_REHEARSE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2 but --gpus 4" in r.stderr


def test_more_gpus_than_visible_fails_before_launch():
    # this container has no GPU: --gpus 2 without a launcher must refuse, not run 1 rank
    r = _run(["--gpus", "2"], {})
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "GPU(s) visible" in r.stderr or "cannot count GPUs from the KFD topology" in r.stderr


def test_kfd_gpu_count_reads_topology_without_hip(tmp_path, monkeypatch):
    """The launcher counts GPUs from the KFD topology (no HIP call before the
    ranks start): nodes with SIMDs are GPUs, the visibility lists cap them,
    and an unreadable topology is None (the launcher then refuses)."""
    sys.path.insert(0, ROOT)
    import bench
    for i, simds in enumerate([0, 1024, 1024, 0, 1024]):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text(f"cpu_cores_count 4\nsimd_count {simds}\nmax_waves_per_simd 8\n")
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert bench.kfd_gpu_count(str(tmp_path)) == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "1")
    assert bench.kfd_gpu_count(str(tmp_path)) == 1
    assert bench.kfd_gpu_count(str(tmp_path / "missing")) is None


def test_gpus_must_be_positive():
    r = _run(["--gpus", "0"], {})
    assert r.returncode != 0 and "--gpus must be >= 1" in r.stderr


def test_steps_must_be_positive():
    r = _run(["--steps", "0"], {})
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_writes_the_counts_as_float64(tmp_path, monkeypatch):
    """--dump-outputs: rank 0 writes DIR/counts.npy (float64, request order);
    other ranks and runs without the option write nothing."""
    import types

    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.delenv("RANK", raising=False)
    out = tmp_path / "dump"
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=None), [1, 2])
    monkeypatch.setenv("RANK", "1")
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(out)), [1, 2])
    assert not out.exists()
    monkeypatch.setenv("RANK", "0")
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(out)), [5412475, 0, (1 << 40) + 1])
    got = np.load(out / "counts.npy")
    assert got.dtype == np.float64 and got.tolist() == [5412475.0, 0.0, float((1 << 40) + 1)]


def test_plain_run_switches_every_other_phase_off():
    """Without --full only the headline steps run: the options of the host
    verification, TopN, serving, configs 4/5, the CPU baseline, the mesh
    breakdown and the page-cache eviction are all off."""
    import types
    sys.path.insert(0, ROOT)
    import bench
    args = types.SimpleNamespace(verify=64, topn_batches=40, cpu_baseline_shards=16, mesh_breakdown=20, cold_load=1,
                                 serve_seconds=5.0, configs="4,5", steps=20, warmup=3)
    bench.headline_only(args)
    assert (args.verify, args.topn_batches, args.cpu_baseline_shards, args.mesh_breakdown, args.cold_load) == (0,) * 5
    assert args.serve_seconds == 0 and args.configs == "" and (args.steps, args.warmup) == (20, 3)
