#!/usr/bin/env python3
"""Measure the per-Namespace counter fold (emurx_nsstat_dev) on 1M-frame batches beside the device
responder and the cache-learning fold on the same batch, and print one JSON line.

Four cases, each a GPU step of its own (a child process under `timeout`; a failing step ends the
run, nothing more is started on the GPU after it):
  c  config C's mix: bench_respond's case d (config C with 5 % echo and ARP requests to its clients
     and a further 2.5 % neighbour solicitations)
  a  config B (64 B UDP, one client): no candidate in the batch
  e  echo requests to the one client of one Namespace: every frame bumps the same counter
  f  the same echo request in 32,768 Namespaces (config D's count), frame i in Namespace i % 32768:
     every 256-frame workgroup holds 256 distinct Namespaces
Cases e and f differ in nothing but the VLAN tags that select the Namespace.

Per case, in one process and on the same device-resident batch: emurx_respond_kinds_dev (every
kind), emurx_learn_dev (both kinds, ev_cap = the distinct keys) and emurx_nsstat_dev (every kind,
ev_cap = the distinct Namespaces, with the outcome arrays of the two).  The timed calls rotate over
--slots copies of the batch at distinct addresses (inputs, records, outcomes and outputs), after two
warm-up rotations, between one HIP event pair: the time is the mean per call of a window of --reps
calls.  Every figure is the median of --windows such windows, the three calls' windows taken in
turn, with the smallest and largest window beside it.  The run also says whether the one-Namespace
batch (e) is slower than the all-distinct batch (f) by more than the spread of the two (the larger
max - min of their windows): if it is, the combining within the workgroup is not working.

    python tools/bench_nsstat.py [--n 1048576] [--reps 40] [--windows 7] [--out profiles/nsstat/bench_nsstat.json]
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

DISTINCT_NS = 32768


def echo_case(n, n_ns):
    """n copies of one 64-byte echo request, frame i in Namespace i % n_ns: QinQ Namespaces on vport
    0 that each hold one client with the same MAC and IPv4 address, so the frames differ in their
    two VLAN ids alone (no checksum covers those)."""
    mac, ip = bytes([0, 0, 1, 0, 0, 0]), bytes([16, 1, 0, 0])
    k = np.arange(n_ns, dtype=np.uint32)
    v0, v1 = 1 + (k >> 8), 1 + (k & 0xFF)
    keys = [F.tunnel_key(0, 0x81000000 | int(a), 0x81000000 | int(b)) for a, b in zip(v0, v1)]
    tmpl = np.frombuffer(BR.echo_request(mac, ip, keys[0], 0, size=64), np.uint8)
    fr = np.tile(tmpl, (n, 1))
    j = np.arange(n) % n_ns
    pcp = tmpl[14] & 0xE0
    fr[:, 14], fr[:, 15] = pcp | (v0[j] >> 8), v0[j] & 0xFF
    fr[:, 18], fr[:, 19] = pcp | (v1[j] >> 8), v1[j] & 0xFF
    stride = 64
    assert fr.shape[1] == stride
    buf = np.zeros(n * stride + 64, np.uint8)
    buf[: n * stride].reshape(n, stride)[:] = fr
    desc = np.zeros(n, abi.DESC_DTYPE)
    desc["off"], desc["len"] = np.arange(n, dtype=np.uint32) * stride, stride
    cl = dict(ns=np.arange(n_ns, dtype=np.int64), cid=np.arange(n_ns), mac=np.tile(np.frombuffer(mac, np.uint8), (n_ns, 1)),
              ipv4=np.tile(np.frombuffer(ip, np.uint8), (n_ns, 1)), ipv6=np.zeros((n_ns, 16), np.uint8))
    return dict(name=f"echo64 in {n_ns} ns", buf=buf, desc=desc, n=n, ns=[(key, i) for i, key in enumerate(keys)], clients=cl)


CASES = {"c": BR.case_d, "a": BR.case_a, "e": lambda n: echo_case(n, 1), "f": lambda n: echo_case(n, DISTINCT_NS)}


def run_case(case, n, reps, slots, windows):
    import torch
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_nsstat needs a HIP device (there is no CPU path)"
    w = CASES[case](n)
    n = len(w["desc"])
    rx = RxPath(0, max_ns=DISTINCT_NS, max_clients=1 << 17, max_frames=n)
    rx.register_all()
    synth.load_tables(w, rx)
    st = torch.cuda.current_stream()

    def dev(a, pad=64):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = torch.zeros(b.size + pad, dtype=torch.uint8, device="cuda")
        t[: b.size] = torch.from_numpy(b.copy()).to("cuda")
        return t

    S = []
    for _ in range(slots):
        S.append(dict(buf=dev(w["buf"]), desc=dev(w["desc"]), rec=torch.zeros(n * 32, dtype=torch.uint8, device="cuda"),
                      hist=torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda"),
                      odesc=torch.empty(n * 8, dtype=torch.uint8, device="cuda"),
                      osrc=torch.empty(n, dtype=torch.int32, device="cuda"),
                      outcome=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      loutcome=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                      done=torch.empty(n, dtype=torch.uint8, device="cuda"),
                      info=torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda"),
                      linfo=torch.zeros(abi.LRN_INFO_WORDS, dtype=torch.int64, device="cuda"),
                      ninfo=torch.zeros(abi.NSS_INFO_WORDS, dtype=torch.int64, device="cuda")))
    for s in S:
        rx.classify_dev(s["buf"], s["desc"], n, s["rec"], None, 0, None, s["hist"], stream=st.cuda_stream)
    # size the outputs: a responder call without room, folds with room for one event
    s0 = S[0]
    rx.respond_dev(s0["buf"], s0["desc"], s0["rec"], n, None, 0, s0["odesc"], s0["osrc"], s0["outcome"], s0["info"],
                   stream=st.cuda_stream, kinds=abi.RSPK_ALL)
    one = torch.empty(96, dtype=torch.uint8, device="cuda")
    rx.learn_dev(s0["buf"], s0["desc"], s0["rec"], n, one, 1, s0["loutcome"], s0["linfo"], stream=st.cuda_stream)
    torch.cuda.synchronize()
    need = int(s0["info"].cpu().numpy()[1])
    keys = max(int(s0["linfo"].cpu().numpy()[1]), 1)
    for s in S:
        s["out"] = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        s["lev"] = torch.empty(keys * 40, dtype=torch.uint8, device="cuda")

    def respond(s):
        rx.respond_dev(s["buf"], s["desc"], s["rec"], n, s["out"], need, s["odesc"], s["osrc"], s["outcome"], s["info"],
                       stream=st.cuda_stream, kinds=abi.RSPK_ALL)

    def learn(s):
        rx.learn_dev(s["buf"], s["desc"], s["rec"], n, s["lev"], keys, s["loutcome"], s["linfo"], stream=st.cuda_stream)

    for s in S:  # the outcome arrays the fold reads: with room for every reply
        respond(s)
        learn(s)
    rx.nsstat_dev(s0["buf"], s0["desc"], s0["rec"], n, s0["outcome"], s0["loutcome"], one, 1, s0["done"], s0["ninfo"],
                  stream=st.cuda_stream)
    torch.cuda.synchronize()
    ev_cap = max(int(s0["ninfo"].cpu().numpy()[1]), 1)
    for s in S:
        s["nev"] = torch.empty(ev_cap * 96, dtype=torch.uint8, device="cuda")

    def nsstat(s):
        rx.nsstat_dev(s["buf"], s["desc"], s["rec"], n, s["outcome"], s["loutcome"], s["nev"], ev_cap, s["done"], s["ninfo"],
                      stream=st.cuda_stream)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for k in range(reps):
            fn(S[k % slots])
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    def stat(a):
        a = np.array(a)
        return {"median": round(float(np.median(a)), 1), "min": round(float(a.min()), 1), "max": round(float(a.max()), 1)}

    for fn in (respond, learn, nsstat):
        for _ in range(2):
            for s in S:
                fn(s)
    rsp_us, lrn_us, nss_us = [], [], []
    for _ in range(windows):  # in turn: what else runs on the machine meets all three alike
        rsp_us.append(window(respond))
        lrn_us.append(window(learn))
        nss_us.append(window(nsstat))
    ninfo = s0["ninfo"].cpu().numpy().view(np.uint64)
    ev = s0["nev"].cpu().numpy()[: int(ninfo[0]) * 96].view(abi.NSSTAT_EV_DTYPE)
    rx.close()
    nm = float(np.median(nss_us))
    return {"case": case, "name": w["name"], "frames": n, "events": int(ninfo[0]), "distinct_ns": int(ninfo[1]),
            "overflow": int(ninfo[2]), "done_1": int(ninfo[3]), "done_2": int(ninfo[4]), "candidates_left": int(ninfo[5]),
            "frames_in_events": int(ev["frames"].sum()), "counters": [int(x) for x in ev["cnt"].sum(axis=0)],
            "nsstat_us": stat(nss_us), "respond_us": stat(rsp_us), "learn_us": stat(lrn_us),
            "nsstat_over_respond": round(nm / float(np.median(rsp_us)), 3),
            "nsstat_over_learn": round(nm / float(np.median(lrn_us)), 3), "reps": reps, "slots": slots, "windows": windows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--slots", type=int, default=4, help="copies of the batch the timed calls rotate over")
    ap.add_argument("--cases", default="caef")
    ap.add_argument("--case", help="(child) run one case in this process")
    ap.add_argument("--step-timeout", type=int, default=170, help="seconds per GPU step")
    ap.add_argument("--dry", action="store_true", help="build the batches only (no GPU): frames and bytes per case")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nsstat" / "bench_nsstat.json"), help="where the JSON line is written too")
    a = ap.parse_args()
    if a.dry:
        for c in a.cases:
            w = CASES[c](a.n)
            print(c, w["name"], len(w["desc"]), int(w["desc"]["len"].astype(np.int64).sum()), len(w["buf"]), len(w["ns"]))
        return 0
    if a.case:
        print(json.dumps(run_case(a.case, a.n, a.reps, a.slots, a.windows)))
        return 0
    res = {"bench": "nsstat", "n": a.n, "cases": []}
    for c in a.cases:
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--case", c, "--n", str(a.n),
                            "--reps", str(a.reps), "--slots", str(a.slots), "--windows", str(a.windows)],
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:  # nothing more on the GPU after a failed step
            res["failed"] = {"case": c, "rc": p.returncode}
            break
        res["cases"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    by = {r["case"]: r["nsstat_us"] for r in res["cases"]}
    if "e" in by and "f" in by:  # one Namespace against all distinct, within this run's own spread
        spread = max(by["e"]["max"] - by["e"]["min"], by["f"]["max"] - by["f"]["min"])
        diff = by["e"]["median"] - by["f"]["median"]
        res["one_ns_vs_distinct"] = {"one_minus_distinct_us": round(diff, 1), "spread_us": round(spread, 1),
                                     "one_ns_not_slower": bool(diff <= spread)}
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
