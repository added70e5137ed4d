"""CPU-side pieces of bench.py (workload synthesis, oracle replay, CPU baseline plumbing) and tracker invariants."""
import importlib.util
import os

import numpy as np
from hypothesis import given, settings, strategies as st

from oracle.strongsort_np import OracleStrongSort
from strongsort_yolo_amd.config import DetectConfig, StrongSortConfig
from strongsort_yolo_amd.engine import letterbox_geometry, scale_geometry
from strongsort_yolo_amd.synth import make_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_workload_and_oracle_replay():
    b = _bench()
    W, H = 640, 480
    g = letterbox_geometry(H, W)
    gs = scale_geometry(g, H, W)
    A = sum((g.out_h // s) * (g.out_w // s) for s in (8, 16, 32))
    wl = b.make_workload(3, W, H, 6, 8, gs, 80, A)
    assert wl["preds"].shape == (8, 84, A) and wl["agt"].shape == (8, A) and wl["pixels"].dtype == np.uint8
    rows = b.oracle_rows(wl, 8, W, H, gs, 80, StrongSortConfig(), DetectConfig())
    assert len(rows) == 8 and rows[-1].shape[1] == 8 and len(rows[-1]) > 0        # confirmed tracks by frame 3
    assert set(b.PRESETS) >= {"c2", "c3", "c4", "c5"} and b.PREFILL >= 103 and b.PREFILL % 16 == 0


@settings(max_examples=15, deadline=None)
@given(st.integers(0, 10_000), st.integers(2, 14))
def test_tracker_invariants(seed, n_ids):
    s = make_stream(seed, 640, 480, n_ids, p_vanish=0.1, vanish_max=6)
    t = OracleStrongSort(StrongSortConfig(max_age=4), "c")
    last_next = 1
    for _ in range(25):
        f = s.next_frame()
        rows = t.update(f.dets, f.feats, (480, 640))
        ids = rows[:, 4].astype(int)
        assert len(set(ids.tolist())) == len(ids)                                  # one row per track
        di = rows[:, 7].astype(int)
        used = di[di >= 0]
        assert len(set(used.tolist())) == len(used) and (used < len(f.dets)).all()  # a detection feeds one track
        assert t.next_id >= last_next                                               # ids are never reused
        last_next = t.next_id
        assert all(tr.state in (1, 2) for tr in t.tracks)                           # deleted tracks are gone
        assert [tr.track_id for tr in t.tracks] == sorted(tr.track_id for tr in t.tracks)
        assert (rows[:, 0] >= 0).all() and (rows[:, 2] <= 639).all() and (rows[:, 3] <= 479).all()


def test_bench_gpus_flag_starts_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher in the environment must come back with n_gpus == 2
    (--gpus was parsed and ignored).  gloo + --dist-check: rendezvous, barrier and the max-over-ranks
    exchange only, no GPU work."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SS_BENCH_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-check"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["dist_check"] is True and res["n_gpus"] == 2 and res["max_over_ranks"] == 2.0
    # under an external launcher the ranks it provides are used as they are
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dist-check"], env=env,
                         capture_output=True, text=True, timeout=600)
    assert json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])["n_gpus"] == 1


def test_rank_affinity_follows_the_gpu_numa_node(tmp_path, monkeypatch):
    """bench.rank_cpus: a rank's cores come from the NUMA node its GPU hangs on (sysfs), shared by the ranks of that node; without
    the information a contiguous slice of the allowed cores."""
    import os
    import types
    import bench
    monkeypatch.setattr(os, "sched_getaffinity", lambda _pid: set(range(16)), raising=False)
    assert bench.rank_cpus(1, 4) == ([4, 5, 6, 7], "contiguous slice")
    # four GPUs: 0, 1 on node 0 (cpus 0-7), 2, 3 on node 1 (cpus 8-15)
    import torch
    props = [types.SimpleNamespace(pci_domain_id=0, pci_bus_id=0x10 + d, pci_device_id=0) for d in range(4)]
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 4)
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda d: props[d])
    for d in range(4):
        p = tmp_path / "bus" / "pci" / "devices" / f"0000:{0x10 + d:02x}:00.0"
        p.mkdir(parents=True)
        (p / "numa_node").write_text(f"{d // 2}\n")
    for k, cl in ((0, "0-7"), (1, "8-15")):
        p = tmp_path / "devices" / "system" / "node" / f"node{k}"
        p.mkdir(parents=True)
        (p / "cpulist").write_text(cl + "\n")
    assert bench.rank_cpus(0, 4, 0, sysfs=str(tmp_path)) == ([0, 1, 2, 3], "NUMA node 0 of GPU 0")
    assert bench.rank_cpus(3, 4, 3, sysfs=str(tmp_path)) == ([12, 13, 14, 15], "NUMA node 1 of GPU 3")
    (tmp_path / "bus" / "pci" / "devices" / "0000:12:00.0" / "numa_node").write_text("-1\n")
    assert bench.rank_cpus(2, 4, 2, sysfs=str(tmp_path))[1] == "contiguous slice"


def test_cpu_baseline_workers_leave_the_gpu_alone():
    """cpu_baseline's per-core workers build the seeded networks, whose torch.random.fork_rng() reads the RNG state of every
    device torch counts (and so opens it).  After the pool initializer torch counts none, on a host with GPUs too."""
    import subprocess
    import sys
    code = ("import sys, torch, bench\n"
            "torch.cuda._raw_device_count_amdsmi = lambda: 8\n"             # a host with eight GPUs
            "assert torch.cuda.device_count() == 8, torch.cuda.device_count()\n"
            "def touched(*a, **k): sys.exit('fork_rng read a device RNG state')\n"
            "torch.cuda.get_rng_state = touched\n"
            "bench._cpu_worker_init()\n"
            "assert torch.cuda.device_count() == 0\n"
            "from strongsort_yolo_amd import nets\n"
            "nets.build_reid(1)\n"
            "assert not torch.cuda.is_initialized()\n")
    env = {k: v for k, v in os.environ.items() if k not in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]


def test_dump_outputs_writes_the_last_timed_step(tmp_path, monkeypatch):
    """--dump-outputs: float32 arrays of the last step's frames only, tracker rows past a frame's count zeroed, the network outputs
    of the last buffer set (head tensor as a fixed seeded sample, valid embedding rows), identical for identical buffers."""
    import types
    import torch
    b = _bench()
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    total, frames, S = 10, 4, 2
    g = torch.Generator().manual_seed(0)
    out_host = torch.rand(total, S, 256, 8, generator=g)
    nout_host = torch.randint(0, 20, (total, S), generator=g, dtype=torch.int32)
    nout_host[-1, 1] = 0
    head = torch.rand(frames * S, 84, 64 * 64, generator=g).half()
    emb = torch.rand(frames * S * 32, 512, generator=g)
    crop_off = torch.tensor([0] * frames * S + [37], dtype=torch.int32)
    last = types.SimpleNamespace(head_out=head, emb_out=emb, crop_off=crop_off)
    other = types.SimpleNamespace(head_out=head + 1, emb_out=emb + 1, crop_off=crop_off)
    pipe = types.SimpleNamespace(bufs=[other, last, other], k=5, nb=3, dev="cpu", Sv=frames * S, pack=True)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), pipe, out_host, nout_host, total, frames)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["embeddings.npy", "head_sample.npy", "track_counts.npy", "track_rows.npy"]
    z = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in z.values())
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 << 20
    cnt = nout_host[total - frames:].numpy()
    assert np.array_equal(z["track_counts"], cnt)
    rows = z["track_rows"]
    assert rows.shape == (frames, S, cnt.max(), 8)
    for f in range(frames):
        for s in range(S):
            n = cnt[f, s]
            assert np.array_equal(rows[f, s, :n], out_host[total - frames + f, s, :n].numpy()) and not rows[f, s, n:].any()
    assert z["head_sample"].shape == (b.DUMP_HEAD_SAMPLE,)
    assert np.isin(z["head_sample"], head.float().flatten().numpy()).all()
    assert np.array_equal(z["embeddings"], emb[:37].numpy())
    for n in names:
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes()
