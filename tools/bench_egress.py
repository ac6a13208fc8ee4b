#!/usr/bin/env python3
"""Measure the egress slots (emurx_egress_*) and the tx planner (emurx_tx_plan_dev), and what they
must not slow down, and print one JSON line.

Steps, each a GPU step of its own (a child process under `timeout`; a failing step ends the run,
nothing more is started on the GPU after it):
  b64k   65,536 x 64 B UDP frames   For each batch: the slot round trip (fill excluded: submit ->
  imix   65,536 IMIX TCP frames     wait, a host clock), and beside it
  b1m    --n x 64 B UDP frames        (a) the device-resident chain plan -> checksum -> framing on the
         same batch between HIP events: what the copies cost;
           (b) orc_tx_checksum + orc_tx_zmq of the CPU oracle on one host core in the same run, with
         the descriptors the planner wrote: the Go-shaped baseline, as bench.py's cpu_baseline is for rx;
           (c) the planner alone and emurx_tx_checksum_dev alone.
         imix against b64k: the planner reads headers only, so `plan_us` of the two must agree within
         the run's own window spread (plan_reads_headers_only).
  base   with --parent-lib: an ingest slot with every answer on (it shares the framing scratch and its
         event hand-off with the egress slots) on bench_respond's case c at 65,536 frames, this tree's
         library and the parent's alternating, --rounds times each.
  bench  with --parent-lib: bench.py --gpus 1 --config B, C and E, --bench-repeats times for each
         library, alternating (the parent's through EMURX_LIB).

Device times are the mean per call of a window of --reps calls between one HIP event pair, host times
the same over a host clock.  Every figure is the median of --windows windows (behind one more that is
dropped) with the smallest and largest beside it, in microseconds.  Against the parent the bar is the
parent's own spread.

    python tools/bench_egress.py [--steps b64k,imix,b1m,base,bench] [--parent-lib PATH] [--out profiles/egress/bench.json] [--keep]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
IMIX = ((64, 7), (594, 4), (1518, 1))  # frame lengths and their shares


def frame(length, proto):
    """A UDP (17) or TCP (6) frame of `length` bytes, checksums valid."""
    from emurx import frames as F
    src, dst = bytes([16, 0, 0, 1]), bytes([48, 0, 0, 1])
    if proto == 17:
        body = bytes(range(256)) * 6
        body = body[: length - 14 - 20 - 8]
        seg = F.udp(1025, 53, body, csum="auto", pseudo=F.ipv4_pseudo(src, dst, 17, 8 + len(body)))
    else:
        body = (bytes(range(256)) * 6)[: length - 14 - 20 - 20]
        seg = F.tcp(1025, 80, body, pseudo=F.ipv4_pseudo(src, dst, 6, 20 + len(body)))
    f = bytes([0, 0, 1, 0, 0, 1]) + bytes([0, 0, 2, 0, 0, 2]) + b"\x08\x00" + F.ipv4(src, dst, proto, seg)
    assert len(f) == length
    return np.frombuffer(f, np.uint8)


def make_batch(n, imix):
    """n frames back to back in send order -> (buf, desc)."""
    from emurx import abi
    if imix:
        lens = np.random.default_rng(7).choice([x for x, _ in IMIX], n, p=np.array([s for _, s in IMIX]) / sum(s for _, s in IMIX))
    else:
        lens = np.full(n, 64)
    lens = lens.astype(np.int64)
    off = np.cumsum(lens) - lens
    buf = np.zeros(int(lens.sum()) + 64, np.uint8)
    for ln in np.unique(lens):
        t = frame(int(ln), 6 if imix else 17)
        idx = off[lens == ln]
        buf[(idx[:, None] + np.arange(ln)[None, :]).reshape(-1)] = np.tile(t, len(idx))
    desc = np.zeros(n, abi.DESC_DTYPE)
    desc["off"], desc["len"], desc["vport"] = off, lens, np.arange(n) % 4
    return buf, desc


def batch_step(n, imix, a):
    import bench_ping as BP
    import pyoracle
    import torch
    from emurx import abi
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_egress needs a HIP device (there is no CPU path)"
    buf, desc = make_batch(n, imix)
    nb = len(buf) - 64
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=n, max_bytes=nb)
    hf, hd = rx.egress_buffer(0)
    hf[:nb], hd[:n] = buf[:nb], desc

    def windows(fn, sync=None):
        us = []
        for _ in range(a.windows + 1):
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            if sync:
                sync()
            us.append((time.perf_counter() - t0) * 1e6 / a.reps)
        return BP.stat(us[1:])

    def slot():
        rx.egress_submit(0, n, nb, 0)
        return rx.egress_wait(0, copy=False)
    for _ in range(3):
        res = slot()
    assert res["n_frames"] == n and not res["status"].any() and int(res["plan_info"][abi.TXP_L4]) == n
    out = {"frames": n, "frame_bytes": nb, "msgs": res["n_msgs"], "msg_bytes": res["bytes"], "slot_us": windows(slot)}

    # the device-resident pieces, between HIP events on the current stream
    st = torch.cuda.current_stream()

    def dev(x, pad=64):
        b = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        t = torch.zeros(b.size + pad, dtype=torch.uint8, device="cuda")
        t[: b.size] = torch.from_numpy(b.copy()).to("cuda")
        return t
    cap = 8 * n + nb
    S = [dict(buf=dev(buf), desc=dev(desc), txd=torch.zeros(n * 16, dtype=torch.uint8, device="cuda"),
              oc=torch.zeros(n, dtype=torch.uint8, device="cuda"), stt=torch.zeros(n, dtype=torch.uint8, device="cuda"),
              info=torch.zeros(16, dtype=torch.int64, device="cuda"), out=torch.zeros(cap + 16, dtype=torch.uint8, device="cuda"),
              off=torch.zeros(n + 1, dtype=torch.int64, device="cuda")) for _ in range(a.slots)]
    plan = lambda s: rx.tx_plan_dev(s["buf"], s["desc"], n, s["txd"], s["oc"], s["info"], 0, stream=st.cuda_stream)  # noqa: E731
    csum = lambda s: rx.tx_checksum_dev(s["buf"], s["txd"], n, s["stt"], stream=st.cuda_stream)  # noqa: E731
    zmq = lambda s: rx.tx_zmq_dev(s["buf"], s["desc"], n, s["out"], cap, s["off"], s["info"][8:], stream=st.cuda_stream)  # noqa: E731

    def chain(s):
        plan(s), csum(s), zmq(s)

    def timed(fn):
        for _ in range(2):
            for s in S:
                fn(s)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.windows + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for r in range(a.reps):
                fn(S[r % len(S)])
            e1.record(st)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        return BP.stat(us[1:])
    out["chain_dev_us"] = timed(chain)
    out["plan_us"] = timed(plan)
    out["checksum_us"] = timed(csum)
    out["zmq_us"] = timed(zmq)
    out["copies_and_slot_overhead_us"] = round(out["slot_us"]["median"] - out["chain_dev_us"]["median"], 1)

    # the Go-shaped baseline on one host core: the oracle's checksum and framing loops
    txd = S[0]["txd"].cpu().numpy().view(abi.TX_DESC_DTYPE)
    pyoracle.build()

    def cpu():
        o, _ = pyoracle.tx_checksum(buf, txd)
        pyoracle.tx_zmq(o, desc)
    reps, a.reps = a.reps, max(1, a.reps // 10)
    out["cpu_one_core_us"] = windows(cpu)
    a.reps = reps
    out["slot_speedup_over_cpu"] = round(out["cpu_one_core_us"]["median"] / out["slot_us"]["median"], 2)
    out.update(reps=a.reps, windows=a.windows, slots=a.slots)
    rx.close()
    return out


def base_step(a):
    """An ingest slot with every answer on, on whichever library EMURX_LIB names."""
    import bench_ftstat as BF
    import bench_respond as BR
    from emurx import abi
    return {"ingest_answers_64k_us": BF.slot_step(BR.case_c(1 << 16), False, a.reps, a.windows, kinds=abi.RSPK_ALL)["us_per_batch"]}


def run_child(a):
    sys.path.insert(0, str(ROOT / "trex-emu_amd"))
    sys.path.insert(0, str(ROOT / "oracle"))
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    if a.case == "b64k":
        return {"step": "b64k", "name": "65,536 x 64 B", **batch_step(1 << 16, False, a)}
    if a.case == "imix":
        return {"step": "imix", "name": "65,536 IMIX (64 / 594 / 1518 at 7 : 4 : 1)", **batch_step(1 << 16, True, a)}
    if a.case == "b1m":
        return {"step": "b1m", "name": f"{a.n} x 64 B", **batch_step(a.n, False, a)}
    return {"step": "base", **base_step(a)}


def main():
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from bench_ping import versus
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="b64k,imix,b1m,base,bench")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--slots", type=int, default=2, help="copies of the batch the timed device calls rotate over")
    ap.add_argument("--rounds", type=int, default=2, help="with --parent-lib: runs of the base step per library, alternating")
    ap.add_argument("--bench-repeats", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=50)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--parent-lib", help="libemurx.so built from the parent commit")
    ap.add_argument("--case", help="(child) run one step in this process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "egress" / "bench.json"), help="where the JSON line is written too")
    ap.add_argument("--keep", action="store_true", help="keep the steps that --out holds from an earlier run and this run does not take")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_child(a)))
        return 0

    def run(cmd, lib):
        env = dict(os.environ)
        if lib:
            env["EMURX_LIB"] = lib
        return subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable] + cmd, stdout=subprocess.PIPE, text=True, env=env)

    def child(case, lib=None):
        p = run([__file__, "--case", case, "--n", str(a.n), "--reps", str(a.reps), "--windows", str(a.windows), "--slots", str(a.slots)], lib)
        return json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else p.returncode

    def bench(config, lib):
        p = run([str(ROOT / "bench.py"), "--gpus", "1", "--config", config, "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)], lib)
        return float(json.loads(p.stdout.strip().splitlines()[-1])["value"]) if p.returncode == 0 else -abs(p.returncode) - 1000

    def alternate(fn, rounds):
        """fn(lib) for the parent's library and this tree's, alternating; the first run that fails
        ends the step (its code is returned) before another is started."""
        vals = {"parent": [], "this": []}
        for _ in range(rounds):
            for t, lib in (("parent", a.parent_lib), ("this", None)):
                v = fn(lib)
                if isinstance(v, int):  # a return code: a child's, or bench()'s negative one
                    return v or -1
                vals[t].append(v)
        return vals

    def child_base(lib):
        return child("base", lib)

    res = {"bench": "egress", "n": a.n, "steps": []}
    for step in a.steps.split(","):
        print(f"step {step}", file=sys.stderr, flush=True)
        if step in ("base", "bench") and not a.parent_lib:  # this tree against the parent only
            continue
        if step in ("b64k", "imix", "b1m"):
            r = child(step)
        elif step == "base":
            r = alternate(child_base, a.rounds)
            if not isinstance(r, int):
                k = "ingest_answers_64k_us"
                r = {"step": "base", "runs": r, k: versus([x[k][f] for x in r["parent"] for f in ("min", "median", "max")],
                                                          [x[k][f] for x in r["this"] for f in ("min", "median", "max")])}
        else:
            r = {"step": "bench", "unit": "Mpkt/s", "steps": a.bench_steps, "warmup": a.bench_warmup}
            for config in ("B", "C", "E"):
                v = alternate(lambda lib: bench(config, lib), a.bench_repeats)  # noqa: B023
                if isinstance(v, int):
                    print(f"bench.py --config {config} failed: {v}", file=sys.stderr, flush=True)
                    r = v
                    break
                r[config] = versus(v["parent"], v["this"])
        if isinstance(r, int):  # nothing more on the GPU after a failed step
            res["failed"] = {"step": step, "rc": r}
            break
        res["steps"].append(r)
    by = {x["step"]: x for x in res["steps"]}
    if "b64k" in by and "imix" in by:  # the planner reads headers only: IMIX no slower than 64 B beyond the windows' spread
        p64, pim = by["b64k"]["plan_us"], by["imix"]["plan_us"]
        spread = max(p64["max"] - p64["min"], pim["max"] - pim["min"])
        res["plan_reads_headers_only"] = {"imix_minus_64B_us": round(pim["median"] - p64["median"], 1), "window_spread_us": round(spread, 1),
                                          "holds": bool(pim["median"] - p64["median"] <= spread)}
    if a.keep and Path(a.out).exists():  # e.g. the batch steps in one run, the bench step in another
        taken = {x["step"] for x in res["steps"]}
        old = json.loads(Path(a.out).read_text())
        res["steps"] = [x for x in old["steps"] if x["step"] not in taken] + res["steps"]
        if "plan_reads_headers_only" in old and "plan_reads_headers_only" not in res:
            res["plan_reads_headers_only"] = old["plan_reads_headers_only"]
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
