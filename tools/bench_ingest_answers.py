#!/usr/bin/env python3
"""Measure the device answers of an ingest slot (emurx_ingest_set_answers) and the counted tx framing
(emurx_tx_zmq_counted_dev), and print one JSON line.

Cases, each a GPU step of its own (a child process under `timeout`; a failing step ends the run,
nothing more is started on the GPU after it):
  off   submit -> wait per batch with answers off: 65,537 frames of 64-byte UDP (config B; the first
        size past the one-launch path) and 1M frames, as messages of 64 frames on one slot.  With
        --parent DIR (a tree of the parent commit with its library built: DIR/emurx, DIR/lib) the
        step runs --rounds times for each of the two trees, alternating, and the run says whether
        this tree is slower than the parent by more than the parent's own run-to-run spread.
  on    the same two inputs with every kind on: no frame is a candidate, so this is the fixed cost
        of the answer stage (respond, the counted framing at count 0 with n_max = the batch, learn,
        nsstat, k_ans_out) on top of `off`.
  echo  65,536 echo requests of 64 bytes to 65,536 clients of one Namespace, every kind on.
  arp   65,536 ARP requests for those clients' addresses, every kind on.
        (on, echo, arp: the time, the bytes k_ans_out moved and the size of the result copy.)
  tx    emurx_tx_zmq_counted_dev against emurx_tx_zmq_dev on 1M frames of 64 bytes in device
        memory: count = n_max = 1M against n = 1M, and count = 1K with n_max = 1M against n = 1K.

Ingest times are a host clock around submit .. wait (the wait ends in a device synchronisation), the
mean per batch of a window of --reps batches after three warm-up batches; framing times the mean
per call between one HIP event pair.  Every figure is the median of --windows windows, with the
smallest and largest beside it, in microseconds.

    python tools/bench_ingest_answers.py [--cases off,on,echo,arp,tx] [--parent DIR] [--out profiles/ingest_answers/bench.json]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SIZES = (65537, 1 << 20)


def stat(a):
    a = np.array(a)
    return {"median": round(float(np.median(a)), 1), "min": round(float(a.min()), 1), "max": round(float(a.max()), 1)}


def zmq_layout(frames):
    """Equal-length frames (an [n, L] array) -> (buf, desc) with each frame behind its 4-byte frame header."""
    from emurx import abi
    n, ln = frames.shape
    rows = np.zeros((n, ln + 4), np.uint8)
    rows[:, 0], rows[:, 2], rows[:, 3] = 0xAA, ln >> 8, ln & 0xFF
    rows[:, 4:] = frames
    buf = np.concatenate([rows.reshape(-1), np.zeros(64, np.uint8)])
    desc = np.zeros(n, abi.DESC_DTYPE)
    desc["off"], desc["len"] = np.arange(n, dtype=np.int64) * (ln + 4) + 4, ln
    return buf, desc


def clients_case(n, kind):
    """n requests, one per client of one untagged Namespace: echo requests to, or ARP requests for, client i."""
    import bench_respond as BR
    from emurx import frames as F
    key = F.tunnel_key(0, 0, 0)
    cid = np.arange(n)
    mac = np.zeros((n, 6), np.uint8)
    mac[:, 2], mac[:, 3], mac[:, 4], mac[:, 5] = 1, cid >> 16, (cid >> 8) & 255, cid & 255
    ip = np.zeros((n, 4), np.uint8)
    ip[:, 0], ip[:, 1], ip[:, 2], ip[:, 3] = 16, 1 + (cid >> 16), (cid >> 8) & 255, cid & 255
    if kind == "echo":
        fr = [BR.echo_request(mac[j].tobytes(), ip[j].tobytes(), key, j) for j in range(n)]
    else:
        fr = [BR.arp_request(ip[j].tobytes(), key, j) for j in range(n)]
    buf, desc = zmq_layout(np.frombuffer(b"".join(fr), np.uint8).reshape(n, len(fr[0])))
    cl = dict(ns=np.zeros(n, np.int64), cid=cid, mac=mac, ipv4=ip, ipv6=np.zeros((n, 16), np.uint8))
    return dict(name=kind, buf=buf, desc=desc, n=n, ns=[(key, 0)], clients=cl)


def r16(x):
    return (int(x) + 15) & ~15


def r256(x):
    return (int(x) + 255) & ~255


def ingest_case(w, kinds, reps, windows):
    """submit -> wait of w's frames as 64-frame messages on slot 0, answers as `kinds` says."""
    import torch
    from emurx import abi, frames as F, synth
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_ingest_answers needs a HIP device (there is no CPU path)"
    zs, msgs = F.zmq_messages(w["buf"], w["desc"], 64)
    n = len(w["desc"])
    rx = RxPath(0, max_ns=16, max_clients=max(2 * len(w["clients"]["cid"]), 16), max_frames=n, max_bytes=len(zs) + 64)
    rx.register_all()
    synth.load_tables(w, rx)
    if kinds:
        rx.ingest_set_answers(0, kinds)
    buf = rx.ingest_buffer(0, len(zs))
    np.copyto(buf, zs)

    def batch():
        rx.ingest_submit(0, msgs)
        return rx.ingest_wait(0, copy=False)
    for _ in range(3):
        res = batch()
    assert res["n"] == n and not res["one_launch"]
    us = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            batch()
        us.append((time.perf_counter() - t0) * 1e6 / reps)
    out = {"frames": n, "msgs": len(msgs), "bytes_in": len(zs), "kinds": kinds, "us_per_batch": stat(us), "reps": reps,
           "windows": windows}
    # the result copy: records, descriptors, queues, status, qoff, histogram, each part on a 256-byte
    # boundary (set_results); with answers three bytes per frame more
    d2h = r256(32 * n) + r256(8 * n) + r256(4 * n) + r256(4 * len(msgs)) + r256(4 * (abi.NUM_QUEUES + 1)) + r256(16 * abi.HIST_BINS)
    if kinds:
        a = rx.ingest_answers(0, n)
        d2h += 3 * r256(n)
        out.update(replies=a["n_replies"], tx_msgs=a["n_tx_msgs"], tx_bytes=a["tx_bytes"], learn_events=len(a["learn_ev"]),
                   ns_events=len(a["ns_ev"]), done_1=int((a["done"] == 1).sum()),
                   ans_out_bytes=288 + r16(8 * (a["n_tx_msgs"] + 1)) + r16(4 * a["n_replies"]) + r16(40 * len(a["learn_ev"])) +
                   r16(96 * len(a["ns_ev"])) + r16(a["tx_bytes"]))
    out["d2h_bytes"] = d2h
    rx.close()
    return out


def tx_case(reps, windows, n=1 << 20, few=1024):
    import torch
    from emurx import abi
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_ingest_answers needs a HIP device (there is no CPU path)"
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=1 << 10)
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(3)
    buf = torch.randint(0, 256, (64 * n + 64,), dtype=torch.uint8, device="cuda", generator=g)
    d = np.zeros(n, abi.DESC_DTYPE)
    d["off"], d["len"] = np.arange(n, dtype=np.int64) * 64, 64
    td = torch.from_numpy(d.view(np.uint8).copy()).to("cuda")
    cap = 72 * n + 64
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    info = torch.empty(2, dtype=torch.int64, device="cuda")
    cnt = {c: torch.tensor([c], dtype=torch.int64, device="cuda") for c in (n, few)}
    calls = {
        "plain_n_1M": lambda: rx.tx_zmq_dev(buf, td, n, out, cap, off, info, stream=st.cuda_stream),
        "counted_1M_of_1M": lambda: rx.tx_zmq_counted_dev(buf, td, n, cnt[n], out, cap, off, info, stream=st.cuda_stream),
        "plain_n_1K": lambda: rx.tx_zmq_dev(buf, td, few, out, cap, off, info, stream=st.cuda_stream),
        "counted_1K_of_1M": lambda: rx.tx_zmq_counted_dev(buf, td, n, cnt[few], out, cap, off, info, stream=st.cuda_stream),
    }
    for _ in range(20):  # past the plain calls' choice of the write's image, which the counted calls take over
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in calls}
    for _ in range(windows):  # in turn: what else runs on the machine meets all of them alike
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                f()
            e1.record(st)
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    res = {"frames": n, "few": few, "image": rx.last_txz(), "reps": reps, "windows": windows}
    res.update({k: stat(v) for k, v in us.items()})
    rx.close()
    return res


def run_child(a):
    sys.path.insert(0, str(Path(a.pkg).resolve()))
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from emurx import abi, synth
    if a.case in ("off", "on"):
        kinds = abi.RSPK_ALL if a.case == "on" else 0
        return {"case": a.case, "udp64": [ingest_case(synth.config_b(n), kinds, a.reps if n > 1 << 17 else 4 * a.reps, a.windows)
                                          for n in SIZES]}
    if a.case in ("echo", "arp"):
        return {"case": a.case, **ingest_case(clients_case(1 << 16, a.case), abi.RSPK_ALL, 4 * a.reps, a.windows)}
    return {"case": "tx", **tx_case(2 * a.reps, a.windows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="off,on,echo,arp,tx")
    ap.add_argument("--reps", type=int, default=20, help="batches per window at 1M frames (four times as many at 64K)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="with --parent: runs of the off case per tree, alternating")
    ap.add_argument("--parent", help="a tree of the parent commit, built (DIR/emurx, DIR/lib/libemurx.so)")
    ap.add_argument("--case", help="(child) run one case in this process")
    ap.add_argument("--pkg", default=str(ROOT / "trex-emu_amd"), help="(child) the tree emurx is imported from")
    ap.add_argument("--step-timeout", type=int, default=170, help="seconds per GPU step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest_answers" / "bench.json"), help="where the JSON line is written too")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_child(a)))
        return 0

    def step(case, pkg):
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--case", case, "--pkg", pkg,
                            "--reps", str(a.reps), "--windows", str(a.windows)], stdout=subprocess.PIPE, text=True)
        return json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else p.returncode

    res = {"bench": "ingest_answers", "cases": []}
    for c in a.cases.split(","):
        plan = [("this", a.pkg)] if not (c == "off" and a.parent) else [(t, p) for _ in range(a.rounds)
                                                                         for t, p in (("parent", a.parent), ("this", a.pkg))]
        runs = []
        for tree, pkg in plan:
            print(f"step {c} ({tree})", file=sys.stderr, flush=True)
            r = step(c, pkg)
            if isinstance(r, int):  # nothing more on the GPU after a failed step
                res["failed"] = {"case": c, "tree": tree, "rc": r}
                break
            runs.append((tree, r))
        if "failed" in res:
            break
        if len(plan) == 1:
            res["cases"].append(runs[0][1])
            continue
        # this tree against the parent, per size: the medians of the alternating runs
        cmp = {"case": "off", "runs": [{"tree": t, **r} for t, r in runs], "vs_parent": []}
        for k, n in enumerate(SIZES):
            med = {t: [r["udp64"][k]["us_per_batch"]["median"] for tt, r in runs if tt == t] for t in ("parent", "this")}
            spread = max(med["parent"]) - min(med["parent"])
            diff = float(np.median(med["this"]) - np.median(med["parent"]))
            cmp["vs_parent"].append({"frames": n, "parent_us": med["parent"], "this_us": med["this"], "parent_spread_us": round(spread, 1),
                                     "this_minus_parent_us": round(diff, 1), "not_slower": bool(diff <= spread)})
        res["cases"].append(cmp)
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
