"""bench.py --gpus N (VERDICT r3 "missing" #2): the flag decides the world size.

* CPU: a --gpus that disagrees with a launcher's WORLD_SIZE exits non-zero before touching a GPU.
* GPU: ``bench.py --gpus 2`` without a launcher starts the two rank processes itself; with
  OFR_DIST_BACKEND=gloo OFR_ONE_DEVICE=1 both ranks share the box's one GPU, and rank 0's JSON line
  reports n_gpus 2 with every query certified and the identities found.

The plain run and --full / --dump-outputs: what a run without --full leaves out (CPU: the parsed
options; GPU: the result line) and what --dump-outputs writes (CPU: files, dtypes, the byte budget,
the seeded sample; GPU: the dump equals the last timed batch's results recomputed in float64).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_gpus_flag_must_match_launcher_world_size():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert "--gpus 2 but WORLD_SIZE=1" in p.stderr


def test_launch_ranks_stops_on_any_rank_failure():
    """a crash of rank 1 while rank 0 is still running (e.g. blocked in a collective) must end
    the launch at once with rank 1's status, not wait for rank 0."""
    import time
    sys.path.insert(0, ROOT)
    import bench
    child = [sys.executable, "-c",
             "import os, sys, time\nif os.environ['RANK'] == '1': sys.exit(3)\ntime.sleep(120)"]
    t0 = time.monotonic()
    assert bench.launch_ranks(2, cmd=child, poll_s=0.05) == 3
    assert time.monotonic() - t0 < 30
    ok = [sys.executable, "-c", "import sys; sys.exit(0)"]
    assert bench.launch_ranks(3, cmd=ok, poll_s=0.05) == 0


def _parse(monkeypatch, *argv):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    """Without --full every extra measurement is off, whatever its own option says; --full keeps the
    extras and their options as they were."""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3", "--stress", "48", "--config3", "1")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_cpu and a.small_batches == "" and a.stress == ""
    assert (a.config1, a.config3, a.config4, a.api) == (0, 0, 0, 0)
    f = _parse(monkeypatch, "--full")
    assert f.full and not f.no_cpu and (f.small_batches, f.stress) == ("32,1", "48,96,192")
    assert (f.config1, f.config3, f.config4, f.api) == (1, 1, 1, 1)
    f = _parse(monkeypatch, "--full", "--no-cpu", "--stress", "", "--config1", "0")
    assert f.no_cpu and f.stress == "" and f.config1 == 0 and f.config3 == 1


def _dump_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def test_dump_outputs_files_and_budget(tmp_path):
    """dump_outputs on host tensors: whole results where they fit, the same seeded row sample on every
    call where they do not, float32 / float64 arrays, never more than DUMP_BUDGET bytes of data."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    B, k, d, ld = 300, 2, 37, 64
    g = torch.Generator().manual_seed(1)
    dist_ = torch.rand((B, k), generator=g, dtype=torch.float64)
    idx = torch.randint(0, 2 ** 40, (B, k), generator=g)
    Qd = torch.randn((B, ld), generator=g)
    bench.dump_outputs(str(tmp_path / "a"), (dist_, idx), Qd, d)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["distances", "indices", "query_feature_rows", "query_features"]
    assert got["distances"].dtype == np.float64 and np.array_equal(got["distances"], dist_.numpy())
    assert got["indices"].dtype == np.float64 and np.array_equal(got["indices"].astype(np.int64), idx.numpy())
    assert got["query_features"].dtype == np.float32
    assert np.array_equal(got["query_feature_rows"], np.arange(B))
    assert np.array_equal(got["query_features"], Qd[:, :d].numpy())

    # a feature matrix past the budget: a sorted sample without repeats, identical on a second call
    B, d = 3000, 9999
    Qd = torch.randn((B, d + 17), generator=g)
    res = (torch.rand((B, 1), generator=g, dtype=torch.float64), torch.arange(B).reshape(B, 1))
    rows = []
    for name in ("b", "c"):
        bench.dump_outputs(str(tmp_path / name), res, Qd, d)
        rows.append(np.load(tmp_path / name / "query_feature_rows.npy").astype(np.int64))
        assert np.array_equal(np.load(tmp_path / name / "query_features.npy"), Qd[rows[-1], :d].numpy())
        assert np.array_equal(np.load(tmp_path / name / "indices.npy")[:, 0], np.arange(B))
        assert _dump_bytes(tmp_path / name) <= bench.DUMP_BUDGET
    assert np.array_equal(rows[0], rows[1]) and 0 < len(rows[0]) < B
    assert np.all(np.diff(rows[0]) > 0) and rows[0][0] >= 0 and rows[0][-1] < B


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_timed_path_computed(tmp_path):
    """A plain run (no --full) at a small shape: the result line carries the headline fields, --steps timed
    steps and none of the extra measurements, and --dump-outputs holds the last timed batch's results:
    the dumped query features are the batch's exact projection, the dumped neighbours its float64
    nearest gallery rows (recomputed here from the same seeds)."""
    import numpy as np
    import torch
    out = tmp_path / "dump"
    N, d, side, B, k, steps = 20_000, 512, 32, 512, 3, 4
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--w", "random",
           "--gallery", str(N), "--dim", str(d), "--side", str(side), "--batch", str(B), "--k", str(k),
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == steps and r["n_gpus"] == 1 and r["unit"] == "queries/s" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0 and abs(r["value"] - B / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    assert sum(r["start_tiers"].values()) == steps
    for key in ("cpu_baseline", "speedup_vs_cpu", "config1", "config3", "stress"):
        assert key not in r, key
    for key in ("config4", "api", "roofline_merge", "certificate_margin_fp6", "feature_profile"):
        assert r[key] is None, key
    assert r["small_batch"] == [] and r["kernels_ms"]["preparation_alone"] is None
    assert _dump_bytes(out) <= 64 * 1000 * 1000

    from opencv_facerecognizer_amd._device import round_up
    from opencv_facerecognizer_amd.synthetic import SEED, IdentityBank, build_gallery, build_projection
    dev = torch.device("cuda", 0)
    per = 10
    P, _ = build_projection(side * side, d, dev)
    bank = IdentityBank(N // per, side, side, device=dev)
    g = build_gallery(P, bank, per, 0, N, N, d, max(32, round_up(d, 32)), dev)
    gq = torch.Generator(device=dev)
    gq.manual_seed(SEED + 7)
    last = (steps - 1) % 3                                  # the pipeline's buffer of the last timed step
    for jb in range(last + 1):
        ids = torch.randint(0, N // per, (B,), generator=gq, device=dev)
    Q = P.project(bank.images(ids, seed=SEED + 99 + last), shift64=g.shift64)[:, :d]
    rows = np.load(out / "query_feature_rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.arange(B))
    feats = np.load(out / "query_features.npy")
    assert feats.dtype == np.float32 and np.array_equal(feats, Q.cpu().numpy())
    D2 = torch.cdist(Q.double(), g.G[:, :d].double(),       # float64 distances to every gallery row
                     compute_mode="donot_use_mm_for_euclid_dist")
    want, _ = torch.topk(D2, k, dim=1, largest=False)
    dd, ii = np.load(out / "distances.npy"), np.load(out / "indices.npy")
    assert dd.dtype == np.float64 and ii.dtype == np.float64 and dd.shape == ii.shape == (B, k)
    np.testing.assert_allclose(dd, want.cpu().numpy(), rtol=1e-9, atol=0)
    at = torch.gather(D2, 1, torch.from_numpy(ii.astype(np.int64)).to(dev)).cpu().numpy()
    np.testing.assert_allclose(at, dd, rtol=1e-9, atol=0)
    assert r["top1_identity_acc"] == float(np.mean(ii[:, 0].astype(np.int64) // per == ids.cpu().numpy()))


@pytest.mark.gpu
def test_bench_gpus_2_spawns_two_ranks():
    env = dict(os.environ, OFR_DIST_BACKEND="gloo", OFR_ONE_DEVICE="1")
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(key, None)
    cmd = [sys.executable, BENCH, "--gpus", "2", "--gallery", "40000", "--batch", "1024", "--steps", "2",
           "--warmup", "1", "--no-cpu", "--stress", "", "--config1", "0", "--small-batches", ""]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 2
    assert r["uncertified_queries_per_step"] == 0.0
    assert r["top1_identity_acc"] == 1.0
