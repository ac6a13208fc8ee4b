"""bench.py's multi-rank launch path without torchrun (the way the driver runs
`python bench.py --gpus N`): N fresh worker processes rendezvous on 127.0.0.1 and rank 0
prints the JSON line; a failing rank ends the whole run with its exit code instead of
leaving the others waiting in a collective.  --launch-check runs the skeleton without a GPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def run(args, env=None, timeout=120):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, env=e, capture_output=True,
                          text=True, timeout=timeout)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("n", [2, 3])
def test_spawned_ranks_gloo(n):
    p = run(["--gpus", str(n), "--backend", "gloo", "--launch-check"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    j = json.loads(lines[0])
    assert j["n_gpus"] == n and j["max_over_ranks"] == float(n) and j["master"] == "127.0.0.1"


@pytest.mark.timeout(180)
def test_stdout_holds_the_json_line_only():
    """What a library writes to the stdout descriptor (RCCL's version banner at communicator
    creation) lands on stderr: the driver reads one JSON line from rank 0's stdout."""
    p = run(["--gpus", "2", "--backend", "gloo", "--launch-check"], env={"EMURX_BENCH_STDOUT_NOISE": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(p.stdout.splitlines()) == 1, p.stdout
    assert json.loads(p.stdout)["launch_check"] == "ok"
    assert p.stderr.count("RCCL version : banner") == 2  # both ranks'


@pytest.mark.timeout(180)
def test_failed_rank_ends_the_run():
    p = run(["--gpus", "2", "--backend", "gloo", "--launch-check"], env={"EMURX_BENCH_FAIL_RANK": "1"})
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])


@pytest.mark.timeout(120)
def test_signalled_launcher_ends_its_ranks():
    """SIGTERM to `bench.py --gpus 2` (the ranks run in sessions of their own) ends every rank
    too, instead of leaving them holding their GPUs; the launcher exits 128 + 15."""
    import os
    import signal
    import time
    import psutil
    p = subprocess.Popen([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--backend", "gloo",
                          "--launch-check"], env=dict(os.environ, EMURX_BENCH_HANG="1"),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    kids = []
    for _ in range(100):
        time.sleep(0.1)
        kids = psutil.Process(p.pid).children(recursive=True)
        if len(kids) >= 2:
            break
    assert len(kids) >= 2, kids
    time.sleep(1.0)
    p.send_signal(signal.SIGTERM)
    assert p.wait(timeout=30) == 128 + signal.SIGTERM
    gone, alive = psutil.wait_procs(kids, timeout=15)
    assert not alive, alive


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_two_rank_exchange_fields(gpu_ok):
    """The bench's N = 2 line over gloo (both ranks on the one GPU): the config-B headline plus the
    Namespace-partitioned exchange timed with the headline's steps and warmup, its per-phase
    device times and the bytes that crossed to the other rank."""
    p = run(["--full", "--gpus", "2", "--backend", "gloo", "--frames", "65536", "--exchange-frames", "65536",
             "--steps", "6", "--warmup", "2", "--batches", "2", "--warmup-seconds", "0.05"], timeout=580)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["value"] > 0
    x = j["namespace_exchange"]
    assert "error" not in x, x
    assert x["steps"] == 6  # the headline's steps, not a side sample
    ph = x["exchange"]["phases"]
    for k in ("source_side_ms", "k_rx_ms", "all_to_all_ms", "owner_lookup_ms"):
        assert ph[k] > 0, (k, ph)
    # a difference of two timings (the source side's group minus k_rx under its own events)
    assert isinstance(ph["owner_count_scan_ms"], float), ph
    # 32-byte heads + tail units (<= 40 bytes per frame crossing to another
    # rank, padding and tail shards included, from 64 + 6 % in round 4)
    assert ph["record_bytes"] == 32
    assert ph["bytes_to_other_ranks"] > ph["payload_bytes_to_other_ranks"] > 0
    assert ph["bytes_per_frame_to_other_ranks"] <= 40, ph
    assert 32 < ph["payload_bytes_per_frame_to_other_ranks"] < 34, ph  # config D: 5 % one-unit tails
    assert ph["xgmi_gbs"] > 0
    # --a2a auto: both transfers timed, their host submit time, the faster one chosen and run
    ch = x["exchange"]["a2a_choice"]
    assert ch["chosen"] in ("equal", "payload") and x["exchange"]["transfer_mode"] == ch["chosen"]
    for k in ("equal", "payload"):
        assert ch[k]["value"] > 0 and ch[k]["host_submit_ms_per_step"] > 0, ch
    # its N = 1 twin, measured in the same job on rank 0: the ratio the >= 6x target is judged by
    t = x["exchange_scaling_target"]
    assert t["n1_value"] > 0 and t["ratio"] > 0 and t["target"] == 6.0 and t["n_gpus"] == 2
    assert abs(t["ratio"] - x["value"] / t["n1_value"]) < 1e-2 * t["ratio"] + 1e-3


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_one_gpu_line_carries_the_exchange(gpu_ok):
    """The --full command's N = 1 line carries namespace_exchange too (config D, partitioned,
    the headline's steps and warmup), so the driver's N = 1 run is the denominator of the
    exchange scaling ratio."""
    p = run(["--full", "--frames", "65536", "--exchange-frames", "65536", "--steps", "6", "--warmup", "2", "--batches", "2",
             "--warmup-seconds", "0.05", "--no-cpu-baseline"], timeout=580)
    assert p.returncode == 0, p.stderr[-3000:]
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    x = j["namespace_exchange"]
    assert "error" not in x, x
    assert j["n_gpus"] == 1 and x["n_gpus"] == 1 and x["steps"] == 6 and x["value"] > 0
    assert x["exchange"]["mode"] == "partitioned" and x["exchange"]["one_stream_steps"]["value"] > 0
    assert "scaling_note" in j["config"]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_dumps_the_last_steps_outputs(gpu_ok, oracle_built, tmp_path):
    """A plain run (no --full) times --steps steps and prints the headline's line without the
    measurements that take runs of their own; --dump-outputs writes the last timed step's
    outputs as float arrays.  Step 2 + 5 - 1 of 2 batch slots reads slot 0, the workload as
    synth makes it: records, queues and counters equal the oracle's on the same frames (20,000
    frames of config C: every frame shape, 79 tiles, the last one partial)."""
    import numpy as np
    from emurx import abi, synth
    from emurx.rx import hist_to_counters
    n = 20000
    p = run(["--gpus", "1", "--config", "C", "--frames", str(n), "--steps", "5", "--warmup", "2", "--batches", "2",
             "--warmup-seconds", "0.05", "--dump-outputs", str(tmp_path)], timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(p.stdout.splitlines()) == 1, p.stdout[-2000:]
    j = json.loads(p.stdout)
    assert j["steps"] == 5 and j["warmup"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0
    for k in ("roofline", "host_inclusive", "namespace_exchange", "cpu_baseline"):
        assert k not in j, k
    assert j["outputs_dumped"]["batch_slot"] == 0
    got = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert set(got) == {"records", "record_rows", "queues", "queue_offsets", "histogram"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    w = synth.config_c(n, rank=0)
    o = oracle_built.Oracle()
    synth.load_tables(w, o)
    orec, oq, oqoff, ocnt = o.rx_batch(w["buf"], w["desc"])
    assert np.array_equal(got["record_rows"], np.arange(n))
    want = np.stack([orec[k].astype(np.float64) for k in abi.REC_DTYPE.names], axis=1)
    assert np.array_equal(got["records"], want)
    assert np.array_equal(got["queues"], oq) and np.array_equal(got["queue_offsets"], oqoff)
    hist = got["histogram"]
    assert np.array_equal(hist, np.round(hist)) and hist[0::2].sum() == n  # one batch's share
    cnt, ocnt = hist_to_counters(hist.astype(np.uint64)), oracle_built.counters_dict(ocnt)
    for k in abi.PARSER_COUNTER_NAMES + ["ref_panic"]:
        assert cnt[k] == ocnt[k], k


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_rank_overlapped_exchange_content(gpu_ok, oracle_built, tmp_path):
    """The bench's own overlapped double-buffer pipeline at N = 2 (gloo, both ranks on the one
    GPU; batch k's parse + all-to-all, then batch k-1's owner lookups, two buffer sets), run for
    4 more steps after the timed ones (--dump-exchange): every rank's resolved records of every
    step equal the oracle's classification of both sources' batches, restricted to the
    Namespaces that rank owns, in (source rank, frame) order -- config D's full tables, 1/2 per
    rank (MapNsT / GetNs thread_ctx.go:139,772-784; ns_ctx.go:262-329)."""
    import numpy as np
    import pyoracle
    from emurx import abi, synth
    from test_gpu_tables import _owners_by_key
    p = run(["--gpus", "2", "--backend", "gloo", "--config", "D", "--frames", "65536", "--steps", "6",
             "--warmup", "2", "--batches", "2", "--warmup-seconds", "0.05", "--no-exchange-run",
             "--dump-exchange", str(tmp_path)], timeout=880)
    assert p.returncode == 0, p.stderr[-3000:]
    o = pyoracle.Oracle()
    synth.load_tables(synth.config_d(1024), o)
    orec = {}
    for r in range(2):
        for j in range(2):
            z = np.load(tmp_path / f"rank{r}_slot{j}.npz")
            orec[(r, j)] = o.rx_batch(z["buf"], z["desc"].view(abi.DESC_DTYPE))[0]
    for r in range(2):
        files = sorted(tmp_path.glob(f"rank{r}_step*.npz"))
        assert len(files) >= 3, files
        for f in files:
            z = np.load(f)
            slot = int(z["slot"])
            got = z["recs"].view(abi.ROUTE_REC_DTYPE)
            want = []
            for s in range(2):
                rec = orec[(s, slot)]
                sel = np.nonzero(_owners_by_key(rec, 2) == r)[0]
                ww = np.zeros(len(sel), abi.ROUTE_REC_DTYPE)
                ww["rec"], ww["src_index"], ww["src_rank"] = rec[sel], sel, s
                want.append(ww)
            want = np.concatenate(want)
            assert len(got) == len(want) and int(z["cnt"].sum()) == len(want), (f.name, len(got), len(want))
            assert got.tobytes() == want.tobytes(), f.name
