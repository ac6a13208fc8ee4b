#!/usr/bin/env python3
"""Measure the device responder (emurx_respond_dev, or emurx_respond_kinds_dev with --kinds) on
1M-frame batches and print one JSON line.

Four cases, each a GPU step of its own (a child process under `timeout`; a failing step ends
the run, nothing more is started on the GPU after it):
  a  config B (64 B UDP, one client): no responder in the batch
  b  64 B ICMP echo requests to 4096 clients: every frame answered
  c  config C with 5 % of the frames replaced by echo requests and ARP requests to its clients
  d  case c with a further 2.5 % (the ARP requests' share) replaced by neighbour solicitations
     for its clients' link-local addresses, half of them duplicate-address-detection probes

Per case, in one process and on the same device-resident batch: the HBM copy ceiling
(emurx_copy_ceiling_dev), k_rx (emurx_classify_dev with every output) and emurx_respond_dev.
The timed calls rotate over R copies of the batch at distinct addresses (inputs, records and
outputs: together well past the 256 MiB last-level cache), after two warm-up rotations, between
one HIP event pair; the time is the mean per call.  Algorithmic bytes of a respond call: 40 B per
frame (record + descriptor) plus, per responder, its frame, its reply and 12 B (output descriptor
+ source index); reported as GB/s and as a fraction of the copy ceiling measured in the process.

    python tools/bench_respond.py [--n 1048576] [--reps 40] [--kinds 15] [--out profiles/respond/x.json]

Kernel time: run one case under the profiler,
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_respond.py --case a
and summarise the trace's k_rsp_* dispatches per call (decide, scan, emit) over the last --reps calls:
    python tools/bench_respond.py --trace DIR [--reps 40]
"""
import argparse
import json
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "trex-emu_amd"))

from emurx import abi, frames as F, synth  # noqa: E402

DUT = bytes([0x00, 0x10, 0x94, 0, 0, 2])


def _tags(key: bytes):
    _, _, v0, v1 = struct.unpack("<HHII", key)
    return b"".join(struct.pack(">HH", v >> 16, (3 << 13) | (v & 0xFFF)) for v in (v0, v1) if v)


def echo_request(mac, ip4, key, seq, size=64):
    body = bytes((seq + k) & 0xFF for k in range(size - 14 - len(_tags(key)) - 28))
    ip = F.ipv4(bytes([48, 0, (seq >> 8) & 0xFF, 1 + seq % 250]), bytes(ip4), 1, F.icmp4(8, 0, seq & 0xFFFF, seq >> 16, body))
    return bytes(mac) + DUT + _tags(key) + b"\x08\x00" + ip


def arp_request(ip4, key, seq):
    a = F.arp(1, DUT, bytes([48, 0, 0, 1 + seq % 250]), bytes(6), bytes(ip4))
    f = b"\xff" * 6 + DUT + _tags(key) + b"\x08\x06" + a
    return f + bytes(max(60 - len(f), 0))


def ns_request(mac, key, seq):
    """A neighbour solicitation for the EUI-64 link-local address of `mac`: from a global source
    with a source link-layer address option, or (odd seq) a duplicate-address-detection probe."""
    mac = bytes(mac)
    tgt = bytes([0xFE, 0x80] + [0] * 6 + [mac[0] ^ 2, mac[1], mac[2], 0xFF, 0xFE, mac[3], mac[4], mac[5]])
    dad = seq & 1
    src = bytes(16) if dad else bytes([0x20, 1, 0x0D, 0xB8] + [0] * 10 + [(seq >> 8) & 0xFF, 1 + seq % 250])
    dst = bytes([0xFF, 2] + [0] * 9 + [1, 0xFF]) + tgt[13:]
    body = bytes(4) + tgt + (b"" if dad else b"\x01\x01" + DUT)
    ic = F.icmp6(135, 0, body, pseudo=F.ipv6_pseudo(src, dst, 4 + len(body), 58))
    return bytes([0x33, 0x33, 0xFF]) + tgt[13:] + DUT + _tags(key) + b"\x86\xdd" + F.ipv6(src, dst, 58, ic, hop=255)


def case_a(n):
    return synth.config_b(n)


def case_b(n, clients=4096):
    """Every frame a 64 B echo request to one of `clients` clients (one untagged Namespace):
    4096 distinct frames, repeated at distinct addresses."""
    key = F.tunnel_key(0, 0, 0)
    cid = np.arange(clients)
    mac = np.zeros((clients, 6), np.uint8)
    mac[:, 2], mac[:, 4], mac[:, 5] = 1, cid >> 8, cid & 255
    ip = np.zeros((clients, 4), np.uint8)
    ip[:, 0], ip[:, 2], ip[:, 3] = 16, cid >> 8, cid & 255
    ip[:, 1] = 1
    uniq = [echo_request(mac[j].tobytes(), ip[j].tobytes(), key, j) for j in range(clients)]
    frames = [uniq[i % clients] for i in range(n)]
    buf, desc = F.pack_frames(frames, [0] * n)
    cl = dict(ns=np.zeros(clients, np.int64), cid=cid, mac=mac, ipv4=ip, ipv6=np.zeros((clients, 16), np.uint8))
    return dict(name="echo64", buf=buf, desc=desc, n=n, ns=[(key, 0)], clients=cl)


def case_c(n, share=0.05, seed=11, ns_share=0.0):
    """Config C with `share` of its frames replaced (same slots of the batch, frames appended to
    the buffer) by echo requests and ARP requests, half each, to random clients of its tables;
    with ns_share, that share of further frames replaced by neighbour solicitations."""
    w = synth.config_c(n)
    rng = np.random.default_rng(seed)
    n_req = int(n * share)
    idx = rng.choice(n, n_req + int(n * ns_share), replace=False)
    is_ns = np.zeros(n, bool)
    is_ns[idx[n_req:]] = True
    idx = np.sort(idx)
    keys = {ns_id: key for key, ns_id in w["ns"]}
    c = w["clients"]
    pick = rng.integers(0, len(c["cid"]), len(idx))
    extra = bytearray()
    base = (len(w["buf"]) + 63) & ~63
    desc = w["desc"].copy()
    for k, (i, j) in enumerate(zip(idx, pick)):
        key = keys[int(c["ns"][j])]
        if is_ns[i]:
            f = ns_request(c["mac"][j].tobytes(), key, k)
        else:
            f = echo_request(c["mac"][j].tobytes(), c["ipv4"][j].tobytes(), key, k) if k & 1 else \
                arp_request(c["ipv4"][j].tobytes(), key, k)
        extra += bytes(4)
        desc[i]["off"], desc[i]["len"], desc[i]["vport"] = base + len(extra), len(f), struct.unpack("<H", key[:2])[0]
        extra += f
    buf = np.zeros(base + len(extra) + 64, np.uint8)
    buf[: len(w["buf"])] = w["buf"]
    buf[base: base + len(extra)] = np.frombuffer(bytes(extra), np.uint8)
    w.update(name="C+5%+NS" if ns_share else "C+5%", buf=buf, desc=desc)
    return w


def case_d(n):
    return case_c(n, ns_share=0.025)


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d}


def run_case(case, n, reps, slots, kinds=None):
    import torch
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_respond needs a HIP device (there is no CPU path)"
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
        s = dict(buf=dev(w["buf"]), desc=dev(w["desc"]), rec=torch.zeros(n * 32, dtype=torch.uint8, device="cuda"),
                 qlist=torch.empty(abi.NUM_QUEUES * qcap, dtype=torch.int32, device="cuda"),
                 tcnt=torch.empty(abi.ntiles(n) * 16, dtype=torch.int32, device="cuda"),
                 hist=torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda"),
                 odesc=torch.empty(n * 8, dtype=torch.uint8, device="cuda"),
                 osrc=torch.empty(n, dtype=torch.int32, device="cuda"),
                 outcome=torch.empty(n, dtype=torch.uint8, device="cuda"),
                 info=torch.zeros(abi.RSP_INFO_WORDS if kinds else 8, dtype=torch.int64, device="cuda"))
        S.append(s)

    def k_rx(s):
        rx.classify_dev(s["buf"], s["desc"], n, s["rec"], s["qlist"], qcap, s["tcnt"], s["hist"], stream=st.cuda_stream)

    for s in S:
        k_rx(s)
    # size the reply buffers with a call that has no room (d_info[1] = bytes needed)
    rx.respond_dev(S[0]["buf"], S[0]["desc"], S[0]["rec"], n, None, 0, S[0]["odesc"], S[0]["osrc"], S[0]["outcome"],
                   S[0]["info"], stream=st.cuda_stream, kinds=kinds)
    torch.cuda.synchronize()
    need = int(S[0]["info"].cpu().numpy()[1])
    for s in S:
        s["out"] = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

    def respond(s):
        rx.respond_dev(s["buf"], s["desc"], s["rec"], n, s["out"], need, s["odesc"], s["osrc"], s["outcome"], s["info"],
                       stream=st.cuda_stream, kinds=kinds)

    def timed(fn):
        for _ in range(2):
            for s in S:
                fn(s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for k in range(reps):
            fn(S[k % slots])
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps  # us per call

    cn = 1 << 30
    src, dst = torch.empty(cn, dtype=torch.uint8, device="cuda"), torch.empty(cn, dtype=torch.uint8, device="cuda")
    copy_us = timed(lambda s: abi.check(lib.emurx_copy_ceiling_dev(dst.data_ptr(), src.data_ptr(), cn, st.cuda_stream), "copy"))
    ceiling = 2 * cn / copy_us / 1e3  # GB/s
    del src, dst
    rx_us = timed(k_rx)
    rsp_us = timed(respond)
    info = S[0]["info"].cpu().numpy().view(np.uint64)
    osrc = S[0]["osrc"].cpu().numpy().view(np.uint32)[: int(info[0])]
    odesc = S[0]["odesc"].cpu().numpy()[: int(info[0]) * 8].view(abi.DESC_DTYPE)
    flen = int(w["desc"]["len"][osrc].astype(np.int64).sum())
    rlen = int(odesc["len"].astype(np.int64).sum())
    fbytes = int(w["desc"]["len"].astype(np.int64).sum())
    rsp_bytes = 40 * n + flen + rlen + 12 * int(info[0])
    # k_rx's algorithmic bytes: frame + descriptor + record + queue entry (108 B per 64 B frame)
    rx.close()
    return {"case": case, "name": w["name"], "kinds": kinds, "outcome_7": int(info[8]) if kinds else 0, "frames": n, "frame_bytes": fbytes, "replies": int(info[0]),
            "reply_bytes_aligned": int(info[1]), "outcomes_1_6": [int(x) for x in info[2:8]],
            "respond_us": round(rsp_us, 1), "respond_alg_bytes": rsp_bytes,
            "respond_gbs": round(rsp_bytes / rsp_us / 1e3, 1), "respond_frac_of_copy": round(rsp_bytes / rsp_us / 1e3 / ceiling, 3),
            "k_rx_us": round(rx_us, 1), "k_rx_alg_bytes": fbytes + 44 * n,
            "k_rx_frac_of_copy": round((fbytes + 44 * n) / rx_us / 1e3 / ceiling, 3),
            "respond_over_k_rx": round(rsp_us / rx_us, 3), "copy_ceiling_gbs": round(ceiling, 1),
            "reps": reps, "slots": slots}


def summarise_trace(path, reps):
    """The k_rsp_* dispatches of a rocprofv3 kernel trace (csv), grouped per call (decide, scan,
    emit): per call the interval from the decide kernel's start to the emit kernel's end and the
    sum of the three kernel times, over the last `reps` calls (the timed ones), in us."""
    import csv
    files = sorted(Path(path).rglob("*kernel_trace.csv")) if Path(path).is_dir() else [Path(path)]
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "k_rsp_" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls = []
    for k in range(0, len(rows) - 2, 3):
        d, s, e = rows[k:k + 3]
        assert "k_rsp_decide" in d[2] and "k_rsp_scan" in s[2] and "k_rsp_emit" in e[2], (d[2], s[2], e[2])
        calls.append(((e[1] - d[0]) / 1e3, [(x[1] - x[0]) / 1e3 for x in (d, s, e)]))
    calls = calls[-reps:]
    span = np.array([c[0] for c in calls])
    ker = np.array([c[1] for c in calls])

    def st(a):
        return {"median": round(float(np.median(a)), 2), "min": round(float(a.min()), 2), "max": round(float(a.max()), 2),
                "mean": round(float(a.mean()), 2), "std": round(float(a.std()), 2)}
    return {"calls": len(calls), "interval_us": st(span), "kernels_sum_us": st(ker.sum(1)), "decide_us": st(ker[:, 0]),
            "scan_us": st(ker[:, 1]), "emit_us": st(ker[:, 2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", type=int, help="EMURX_RSPK_* mask: emurx_respond_kinds_dev (default: emurx_respond_dev)")
    ap.add_argument("--trace", help="summarise the k_rsp_* kernels of a rocprofv3 kernel trace (csv file or directory)")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--slots", type=int, default=4, help="copies of the batch the timed calls rotate over")
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--case", help="(child) run one case in this process")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per GPU step")
    ap.add_argument("--dry", action="store_true", help="build the batches only (no GPU): frames and bytes per case")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(summarise_trace(a.trace, a.reps)))
        return 0
    if a.dry:
        for c in a.cases:
            w = CASES[c](a.n)
            print(c, w["name"], len(w["desc"]), int(w["desc"]["len"].astype(np.int64).sum()), len(w["buf"]))
        return 0
    if a.case:
        print(json.dumps(run_case(a.case, a.n, a.reps, a.slots, a.kinds)))
        return 0
    res = {"bench": "respond", "n": a.n, "cases": []}
    for c in a.cases:
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--case", c, "--n", str(a.n),
                            "--reps", str(a.reps), "--slots", str(a.slots)] + (["--kinds", str(a.kinds)] if a.kinds else []),
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
