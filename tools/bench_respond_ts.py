#!/usr/bin/env python3
"""Measure emurx_respond_ts_dev (the ICMPv4 timestamp reply) against emurx_respond_kinds_dev on
1M-frame batches in device memory and print one JSON line.

Batches (bench_respond.py builds the first two), each a GPU step of its own (a child process under
`timeout`; a failing step ends the run, nothing more is started on the GPU after it):
  a  config B (64 B UDP, one client): no candidate in the batch
  b  config C with 5 % of the frames replaced by echo requests and ARP requests
  d  62-byte timestamp requests to one client (the reference's TestPluginIcmp2 frame)
  e  62-byte echo requests to the same client
Rows: (a), (b) = emurx_respond_kinds_dev(15) on batches a and b; (c.a), (c.b) = emurx_respond_ts_dev(31)
on the same batches in the same process; (d), (e) = emurx_respond_ts_dev(31) on batches d and e.
A library without the new entry point (the parent commit's, given through EMURX_LIB) gives rows (a)
and (b) alone: the yardstick for "the existing entry points did not get slower".

The timed calls rotate over four copies of the batch at distinct addresses (inputs, records and
outputs), after two warm-up rotations; a window is the mean per call of --reps calls between one HIP
event pair; a row is the median of --windows such windows with the smallest and the largest.
Algorithmic bytes of a call: 40 B per frame (record + descriptor) plus, per reply, its frame, the
reply and 12 B (output descriptor + source index); a timestamp reply's frame is read once, like an
echo reply's, and its checksum is one more 2-byte store.

    python tools/bench_respond_ts.py [--n 1048576] [--steps abde] [--out run.json]
    EMURX_LIB=<parent's libemurx.so> python tools/bench_respond_ts.py --steps ab --out parent1.json
    python tools/bench_respond_ts.py --merge this1.json parent1.json ... --out profiles/respond_ts/bench.json

Which launch a difference lands in: run one step under the profiler,
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_respond_ts.py --step b
and summarise the k_rsp_* dispatches of the timed calls per entry point (decide, scan, emit):
    python tools/bench_respond_ts.py --trace DIR
"""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "trex-emu_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import bench_respond as B  # noqa: E402
from emurx import abi, frames as F, synth  # noqa: E402

KEY = F.tunnel_key(1, 0x81000001, 0x81000002)
MAC, IP4 = bytes([0, 0, 1, 0, 0, 0]), bytes([16, 0, 0, 0])
TIME = 43_200_000


def ts_request(seq):
    ic = F.icmp4(13, 0, 1, seq & 0xFFFF, bytes([seq & 0xFF, (seq >> 8) & 0xFF, 0, 0]) + bytes(8))
    ip = F.ipv4(bytes([48, 0, (seq >> 8) & 0xFF, 1 + seq % 250]), IP4, 1, ic, ttl=128, ident=0xCC)
    return MAC + B.DUT + B._tags(KEY) + b"\x08\x00" + ip


def one_client(n, make, name):
    uniq = [make(j) for j in range(4096)]
    assert all(len(f) == 62 for f in uniq)
    buf, desc = F.pack_frames([uniq[i % 4096] for i in range(n)], [1] * n)
    cl = dict(ns=np.zeros(1, np.int64), cid=np.zeros(1, np.int64), mac=np.frombuffer(MAC, np.uint8).reshape(1, 6).copy(),
              ipv4=np.frombuffer(IP4, np.uint8).reshape(1, 4).copy(), ipv6=np.zeros((1, 16), np.uint8))
    return dict(name=name, buf=buf, desc=desc, n=n, ns=[(KEY, 0)], clients=cl)


BATCHES = {"a": B.case_a, "b": B.case_c, "d": lambda n: one_client(n, ts_request, "ts62"),
           "e": lambda n: one_client(n, lambda j: B.echo_request(MAC, IP4, KEY, j, size=62), "echo62")}


def run_step(step, n, reps, windows, slots):
    import torch
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_respond_ts needs a HIP device (there is no CPU path)"
    lib = abi.load()
    has_ts = hasattr(lib, "emurx_respond_ts_dev") and "EMURX_LIB" not in os.environ
    w = BATCHES[step](n)
    n = len(w["desc"])
    rx = RxPath(0, max_ns=4096, max_clients=1 << 17, max_frames=n)
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
        s = dict(buf=dev(w["buf"]), desc=dev(w["desc"]), rec=torch.zeros(n * 32, dtype=torch.uint8, device="cuda"),
                 hist=torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda"),
                 odesc=torch.empty(n * 8, dtype=torch.uint8, device="cuda"), osrc=torch.empty(n, dtype=torch.int32, device="cuda"),
                 outcome=torch.empty(n, dtype=torch.uint8, device="cuda"),
                 info=torch.zeros(abi.RSP_INFO_WORDS, dtype=torch.int64, device="cuda"))
        rx.classify_dev(s["buf"], s["desc"], n, s["rec"], None, 0, None, s["hist"], stream=st.cuda_stream)
        S.append(s)

    def call(s, ts, out, cap):
        rx.respond_dev(s["buf"], s["desc"], s["rec"], n, out, cap, s["odesc"], s["osrc"], s["outcome"], s["info"],
                       stream=st.cuda_stream, kinds=abi.RSPK_ALL_TS if ts else abi.RSPK_ALL, ip_time=TIME if ts else None)

    def measure(ts):
        call(S[0], ts, None, 0)  # a call without room sizes the reply buffers: d_info[1] = bytes needed
        torch.cuda.synchronize()
        need = int(S[0]["info"].cpu().numpy()[1])
        outs = [torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") for _ in S]
        for _ in range(2):
            for s, o in zip(S, outs):
                call(s, ts, o, need)
        win = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for k in range(reps):
                call(S[k % slots], ts, outs[k % slots], need)
            e1.record(st)
            torch.cuda.synchronize()
            win.append(round(e0.elapsed_time(e1) * 1e3 / reps, 2))  # us per call
        info = S[0]["info"].cpu().numpy().view(np.uint64)
        k = int(info[0])
        osrc = S[0]["osrc"].cpu().numpy().view(np.uint32)[:k]
        odesc = S[0]["odesc"].cpu().numpy()[: k * 8].view(abi.DESC_DTYPE)
        flen, rlen = int(w["desc"]["len"][osrc].astype(np.int64).sum()), int(odesc["len"].astype(np.int64).sum())
        n_ts = int(info[1 + abi.RSP_TS]) if ts else 0
        alg = 40 * n + flen + rlen + 12 * k
        med = float(np.median(win))
        del outs
        return {"call": "emurx_respond_ts_dev(31)" if ts else "emurx_respond_kinds_dev(15)", "batch": w["name"], "frames": n,
                "replies": k, "ts_replies": n_ts, "outcomes_1_9": [int(x) for x in info[2:11]], "windows_us": win,
                "median_us": round(med, 2), "min_us": min(win), "max_us": max(win), "alg_bytes": alg,
                "gbs": round(alg / med / 1e3, 1)}

    rows = {}
    if step in "ab":
        rows["(%s)" % step] = measure(False)
        if has_ts:
            rows["(c.%s)" % step] = measure(True)
    elif has_ts:
        rows["(%s)" % step] = measure(True)
    rx.close()
    return rows


def summarise_trace(path, reps, windows, slots):
    """The k_rsp_* dispatches of a rocprofv3 kernel trace (csv), three per call; the calls of the
    entry point with the timestamp kind are those whose scan kernel is k_rsp_scan<true>.  Per entry
    point the medians, over its timed calls (the last reps * windows), of the three kernels, of their
    sum and of the interval from the decide kernel's start to the emit kernel's end, in us."""
    import csv
    files = sorted(Path(path).rglob("*kernel_trace.csv")) if Path(path).is_dir() else [Path(path)]
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "k_rsp_" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls = {}
    for k in range(0, len(rows) - 2, 3):
        d, s, e = rows[k:k + 3]
        assert "k_rsp_decide" in d[2] and "k_rsp_scan" in s[2] and "k_rsp_emit" in e[2], (d[2], s[2], e[2])
        who = "emurx_respond_ts_dev(31)" if "k_rsp_scan<true>" in s[2] or "k_rsp_scanILb1" in s[2] else "emurx_respond_kinds_dev(15)"
        calls.setdefault(who, []).append([(x[1] - x[0]) / 1e3 for x in (d, s, e)] + [(e[1] - d[0]) / 1e3])
    out = {}
    for who, c in calls.items():
        a = np.array(c[-reps * windows:])
        med = lambda v: round(float(np.median(v)), 2)  # noqa: E731
        out[who] = {"calls": len(a), "decide_us": med(a[:, 0]), "scan_us": med(a[:, 1]), "emit_us": med(a[:, 2]),
                    "kernels_sum_us": med(a[:, :3].sum(1)), "interval_us": med(a[:, 3])}
    return out


def st3(v):
    return {"median": round(float(np.median(v)), 2), "min": min(v), "max": max(v)}


def merge(files):
    """Runs of this tree and of the parent -> the table's figures and the two conditions' numbers."""
    runs = [json.loads(Path(f).read_text()) for f in files]
    out = {"bench": "respond_ts", "runs": runs, "rows": {}}
    for who in ("tree", "parent"):
        for r in ("(a)", "(b)", "(c.a)", "(c.b)", "(d)", "(e)"):
            med = [x["rows"][r]["median_us"] for x in runs if x["library"] == who and r in x["rows"]]
            if med:
                out["rows"]["%s %s" % (who, r)] = dict(st3(med), runs=med)
    rows = out["rows"]
    for r in ("(a)", "(b)"):
        if "tree " + r in rows and "parent " + r in rows:
            p = rows["parent " + r]
            out["condition_1 " + r] = {"tree_minus_parent_us": round(rows["tree " + r]["median"] - p["median"], 2),
                                       "parent_spread_us": round(p["max"] - p["min"], 2)}
        c = "(c.%s)" % r[1]
        if "tree " + c in rows:
            out["condition_2 " + c] = {"ts_minus_kinds_us": round(rows["tree " + c]["median"] - rows["tree " + r]["median"], 2)}
    if "tree (d)" in rows and "tree (e)" in rows:
        out["d_over_e"] = round(rows["tree (d)"]["median"] / rows["tree (e)"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--slots", type=int, default=4, help="copies of the batch the timed calls rotate over")
    ap.add_argument("--steps", default="abde")
    ap.add_argument("--step", help="(child) run one step in this process")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per GPU step")
    ap.add_argument("--trace", help="summarise the k_rsp_* kernels of a rocprofv3 kernel trace (csv file or directory)")
    ap.add_argument("--merge", nargs="+", help="merge the JSON files of several runs into the committed summary")
    ap.add_argument("--out", help="also write the JSON to this file")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(summarise_trace(a.trace, a.reps, a.windows, a.slots)))
        return 0
    if a.step:
        print(json.dumps(run_step(a.step, a.n, a.reps, a.windows, a.slots)))
        return 0
    if a.merge:
        res = merge(a.merge)
    else:
        res = {"bench": "respond_ts", "library": "parent" if "EMURX_LIB" in os.environ else "tree", "n": a.n, "reps": a.reps,
               "rows": {}}
        for c in a.steps:
            p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--step", c, "--n", str(a.n),
                                "--reps", str(a.reps), "--windows", str(a.windows), "--slots", str(a.slots)],
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:  # nothing more on the GPU after a failed step
                res["failed"] = {"step": c, "rc": p.returncode}
                break
            res["rows"].update(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps(res, indent=1 if a.merge else None)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
