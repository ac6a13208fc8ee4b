#!/usr/bin/env python3
"""Measure the cache-learning fold (emurx_learn_dev) on 1M-frame batches beside the device
responder, k_rx and the HBM copy ceiling, and print one JSON line.

Five cases, each a GPU step of its own (a child process under `timeout`; a failing step ends the
run, nothing more is started on the GPU after it):
  a  config B (64 B UDP, one client): no candidate in the batch
  c  bench_respond's case c: config C with 5 % echo and ARP requests to its clients
  d  bench_respond's case d: case c with a further 2.5 % neighbour solicitations
  e  ARP requests from one sender: one key, the contention case
  f  ARP requests from as many distinct senders as frames: every key its own slot

Per case, in one process and on the same device-resident batch: the copy ceiling
(emurx_copy_ceiling_dev), k_rx (emurx_classify_dev with every output), emurx_respond_kinds_dev
(every kind) and emurx_learn_dev (both kinds, ev_cap = the distinct keys).  The timed calls rotate
over --slots copies of the batch at distinct addresses (inputs, records and outputs), after two
warm-up rotations, between one HIP event pair: the time is the mean per call of a window of
--reps calls.  Every figure is the median of --windows such windows, the responder's and the
fold's taken alternately, with the smallest and largest window beside it.  Algorithmic bytes of a
learn call: 16 B of record per frame and one outcome byte, plus per candidate the other half of
its record, its descriptor and 32 B of its frame, plus 40 B per event.

    python tools/bench_learn.py [--n 1048576] [--reps 40] [--windows 7] [--out profiles/learn/x.json]

Kernel time: run one case under the profiler,
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_learn.py --case e
and summarise the trace's k_lrn_* and k_rsp_* dispatches per call over the last calls:
    python tools/bench_learn.py --trace DIR
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "trex-emu_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import bench_respond as BR  # noqa: E402
from emurx import abi, frames as F, synth  # noqa: E402


def arp_case(n, senders):
    """n 60-byte ARP requests for the one client's address, sender i % senders (its MAC and its IP
    both count up): one untagged Namespace on vport 0."""
    key = F.tunnel_key(0, 0, 0)
    mac, ip = bytes([0, 0, 1, 0, 0, 0]), bytes([16, 1, 0, 0])
    tmpl = np.frombuffer(BR.arp_request(ip, key, 0), np.uint8)
    fr = np.tile(tmpl, (n, 1))
    j = (np.arange(n) % senders).astype(np.uint32)
    for col, sh in ((3, 16), (4, 8), (5, 0)):
        fr[:, 6 + col] = fr[:, 22 + col] = (j >> sh) & 0xFF        # Ethernet source, sender hardware address
    fr[:, 28], fr[:, 29], fr[:, 30], fr[:, 31] = 48, (j >> 16) & 0xFF, (j >> 8) & 0xFF, j & 0xFF  # sender IP
    stride = 64
    buf = np.zeros(n * stride + 64, np.uint8)
    buf[: n * stride].reshape(n, stride)[:, : fr.shape[1]] = fr
    desc = np.zeros(n, abi.DESC_DTYPE)
    desc["off"], desc["len"] = np.arange(n, dtype=np.uint32) * stride, fr.shape[1]
    cl = dict(ns=np.zeros(1, np.int64), cid=np.arange(1), mac=np.frombuffer(mac, np.uint8).reshape(1, 6).copy(),
              ipv4=np.frombuffer(ip, np.uint8).reshape(1, 4).copy(), ipv6=np.zeros((1, 16), np.uint8))
    return dict(name=f"arp x{senders}", buf=buf, desc=desc, n=n, ns=[(key, 0)], clients=cl)


CASES = {"a": BR.case_a, "c": BR.case_c, "d": BR.case_d, "e": lambda n: arp_case(n, 1), "f": lambda n: arp_case(n, n)}


def run_case(case, n, reps, slots, windows):
    import torch
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_learn needs a HIP device (there is no CPU path)"
    w = CASES[case](n)
    n = len(w["desc"])
    rx = RxPath(0, max_ns=4096, max_clients=1 << 17, max_frames=n)
    rx.register_all()
    synth.load_tables(w, rx)
    st = torch.cuda.current_stream()
    lib = abi.load()

    def dev(a, pad=64):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = torch.zeros(b.size + pad, dtype=torch.uint8, device="cuda")
        t[: b.size] = torch.from_numpy(b.copy()).to("cuda")
        return t

    qcap = abi.queue_cap(n)
    S = []
    for _ in range(slots):
        S.append(dict(buf=dev(w["buf"]), desc=dev(w["desc"]), rec=torch.zeros(n * 32, dtype=torch.uint8, device="cuda"),
                      qlist=torch.empty(abi.NUM_QUEUES * qcap, dtype=torch.int32, device="cuda"),
                      tcnt=torch.empty(abi.ntiles(n) * 16, dtype=torch.int32, device="cuda"),
                      hist=torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda"),
                      odesc=torch.empty(n * 8, dtype=torch.uint8, device="cuda"),
                      osrc=torch.empty(n, dtype=torch.int32, device="cuda"),
                      outcome=torch.empty(n, dtype=torch.uint8, device="cuda"),
                      loutcome=torch.empty(n, dtype=torch.uint8, device="cuda"),
                      info=torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda"),
                      linfo=torch.zeros(abi.LRN_INFO_WORDS, dtype=torch.int64, device="cuda")))

    def k_rx(s):
        rx.classify_dev(s["buf"], s["desc"], n, s["rec"], s["qlist"], qcap, s["tcnt"], s["hist"], stream=st.cuda_stream)

    for s in S:
        k_rx(s)
    # size the outputs: a responder call without room, a fold with room for one event
    s0 = S[0]
    rx.respond_dev(s0["buf"], s0["desc"], s0["rec"], n, None, 0, s0["odesc"], s0["osrc"], s0["outcome"], s0["info"],
                   stream=st.cuda_stream, kinds=abi.RSPK_ALL)
    one = torch.empty(40, dtype=torch.uint8, device="cuda")
    rx.learn_dev(s0["buf"], s0["desc"], s0["rec"], n, one, 1, s0["loutcome"], s0["linfo"], stream=st.cuda_stream)
    torch.cuda.synchronize()
    need = int(s0["info"].cpu().numpy()[1])
    keys = int(s0["linfo"].cpu().numpy()[1])
    ev_cap = max(keys, 1)
    for s in S:
        s["out"] = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        s["ev"] = torch.empty(ev_cap * 40, dtype=torch.uint8, device="cuda")

    def respond(s):
        rx.respond_dev(s["buf"], s["desc"], s["rec"], n, s["out"], need, s["odesc"], s["osrc"], s["outcome"], s["info"],
                       stream=st.cuda_stream, kinds=abi.RSPK_ALL)

    def learn(s):
        rx.learn_dev(s["buf"], s["desc"], s["rec"], n, s["ev"], ev_cap, s["loutcome"], s["linfo"], stream=st.cuda_stream)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for k in range(reps):
            fn(S[k % slots])
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    def warm(fn):
        for _ in range(2):
            for s in S:
                fn(s)

    def stat(a):
        a = np.array(a)
        return {"median": round(float(np.median(a)), 1), "min": round(float(a.min()), 1), "max": round(float(a.max()), 1)}

    cn = 1 << 30
    src, dst = torch.empty(cn, dtype=torch.uint8, device="cuda"), torch.empty(cn, dtype=torch.uint8, device="cuda")
    copy = lambda s: abi.check(lib.emurx_copy_ceiling_dev(dst.data_ptr(), src.data_ptr(), cn, st.cuda_stream), "copy")  # noqa: E731
    warm(copy)
    copy_us = [window(copy) for _ in range(3)]
    del src, dst
    warm(k_rx)
    rx_us = [window(k_rx) for _ in range(3)]
    warm(respond)
    warm(learn)
    rsp_us, lrn_us = [], []
    for _ in range(windows):  # alternately: what else runs on the machine meets both alike
        rsp_us.append(window(respond))
        lrn_us.append(window(learn))
    linfo = s0["linfo"].cpu().numpy().view(np.uint64)
    info = s0["info"].cpu().numpy().view(np.uint64)
    lo = s0["loutcome"].cpu().numpy()
    cand = int((lo != 0).sum())  # a lower bound of the candidates: those with an outcome
    alg = 17 * n + cand * (16 + 8 + 32) + 40 * int(linfo[0])
    ceiling = 2 * cn / float(np.median(copy_us)) / 1e3
    rx.close()
    lm = float(np.median(lrn_us))
    return {"case": case, "name": w["name"], "frames": n, "events": int(linfo[0]), "distinct": int(linfo[1]),
            "overflow": int(linfo[2]), "learn_outcomes_1_5": [int(x) for x in linfo[3:8]], "replies": int(info[0]),
            "learn_us": stat(lrn_us), "respond_us": stat(rsp_us), "k_rx_us": stat(rx_us),
            "learn_over_respond": round(lm / float(np.median(rsp_us)), 3), "learn_over_k_rx": round(lm / float(np.median(rx_us)), 3),
            "learn_alg_bytes": alg, "learn_gbs": round(alg / lm / 1e3, 1), "copy_ceiling_gbs": round(ceiling, 1),
            "learn_frac_of_copy": round(alg / lm / 1e3 / ceiling, 3), "reps": reps, "slots": slots, "windows": windows}


def summarise_trace(path, last):
    """The k_lrn_* (decide, mark, scan, emit) and k_rsp_* (decide, scan, emit) dispatches of a
    rocprofv3 kernel trace (csv), grouped per call: per call the interval from the first kernel's
    start to the last kernel's end and the kernels' own times, over the last `last` calls, in us."""
    import csv
    files = sorted(Path(path).rglob("*kernel_trace.csv")) if Path(path).is_dir() else [Path(path)]
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()

    def st(a):
        a = np.array(a)
        return {"median": round(float(np.median(a)), 2), "min": round(float(a.min()), 2), "max": round(float(a.max()), 2)}

    out = {}
    for tag, names in (("learn", ["k_lrn_decide", "k_lrn_mark", "k_lrn_scan", "k_lrn_emit"]),
                       ("respond", ["k_rsp_decide", "k_rsp_scan", "k_rsp_emit"])):
        sel = [r for r in rows if names[0][:6] in r[2]]
        calls = []
        for k in range(0, len(sel) - len(names) + 1, len(names)):
            g = sel[k:k + len(names)]
            assert all(nm in x[2] for nm, x in zip(names, g)), [x[2] for x in g]
            calls.append(((g[-1][1] - g[0][0]) / 1e3, [(x[1] - x[0]) / 1e3 for x in g]))
        calls = calls[-last:]
        if calls:
            ker = np.array([c[1] for c in calls])
            out[tag] = dict(calls=len(calls), interval_us=st([c[0] for c in calls]), kernels_sum_us=st(ker.sum(1)),
                            **{nm + "_us": st(ker[:, j]) for j, nm in enumerate(names)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", help="summarise the k_lrn_* / k_rsp_* kernels of a rocprofv3 kernel trace (csv file or directory)")
    ap.add_argument("--last", type=int, default=120, help="calls of the trace to summarise (the timed windows come last)")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--slots", type=int, default=4, help="copies of the batch the timed calls rotate over")
    ap.add_argument("--cases", default="acdef")
    ap.add_argument("--case", help="(child) run one case in this process")
    ap.add_argument("--step-timeout", type=int, default=170, help="seconds per GPU step")
    ap.add_argument("--dry", action="store_true", help="build the batches only (no GPU): frames and bytes per case")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(summarise_trace(a.trace, a.last)))
        return 0
    if a.dry:
        for c in a.cases:
            w = CASES[c](a.n)
            print(c, w["name"], len(w["desc"]), int(w["desc"]["len"].astype(np.int64).sum()), len(w["buf"]))
        return 0
    if a.case:
        print(json.dumps(run_case(a.case, a.n, a.reps, a.slots, a.windows)))
        return 0
    res = {"bench": "learn", "n": a.n, "cases": []}
    for c in a.cases:
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--case", c, "--n", str(a.n),
                            "--reps", str(a.reps), "--slots", str(a.slots), "--windows", str(a.windows)],
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:  # nothing more on the GPU after a failed step
            res["failed"] = {"case": c, "rc": p.returncode}
            break
        res["cases"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
