#!/usr/bin/env python3
"""Measure the send side of ping on the device (emurx_pingtx_*, emurx_egress_submit_ping) against the
same echo requests submitted as plain frames through emurx_egress_submit, and print one JSON line.

Cases, each a GPU step of its own (a child process under `timeout`; a failing step ends the run,
nothing more is started on the GPU after it):
  a      65,536 requests of count 1 over 65,536 distinct 70-byte templates, on an egress slot
  b      1,024 requests of count 64 over 1,024 templates: the same 65,536 frames
  d      a tick-sized batch: 2,048 requests of count 1 over 2,048 templates
         For each: the slot round trip (fill excluded: submit -> wait, a host clock) with requests,
         `ping_slot_us`, and with the very frames the generator made, taken from its messages and
         submitted as plain frames (70 bytes back to back, 8-byte descriptors), `plain_slot_us`: the
         parent's path.  The two results' messages are compared byte for byte before anything is timed.
  c      emurx_pingtx_dev alone on the requests of a and of b, between HIP events.

Host times are the mean per call of a window of --reps calls over a host clock, device times the same
between one HIP event pair.  Every figure is the median of --windows windows (behind one more that is
dropped) with the smallest and largest beside it, in microseconds.  `faster_beyond_plain_spread` says
whether the requests' median is below the plain path's by more than the plain path's own window spread.

    python tools/bench_pingtx.py [--steps a,b,c,d] [--out profiles/pingtx/bench.json]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
MAGIC = 0xC15C0C15C0BE5BE5
CASES = {"a": (1 << 16, 1), "b": (1 << 10, 64), "d": (1 << 11, 1)}  # requests, count


def template(i):
    """Ping i's packet: two VLAN tags, IPv4, an echo request with 20 bytes of payload: 70 bytes,
    icmp_off 42 (plugins/icmp/icmp.go:208-237 with the simulation's payload size)."""
    from emurx import frames as F
    pay = MAGIC.to_bytes(8, "big") + bytes(12)
    ip = F.ipv4(bytes([16, 0, (i >> 8) & 0xFF, i & 0xFF]), bytes([48, 0, 0, 1]), 1, F.icmp4(8, 0, 0x1234, i & 0xFFFF, pay))
    t = bytes(6) + bytes([0, 0, 1, (i >> 16) & 0xFF, (i >> 8) & 0xFF, i & 0xFF]) + bytes([0x81, 0, 0, 1, 0x81, 0, 0, 2, 8, 0]) + ip
    assert len(t) == 70
    return t


def setup(n_req, count):
    import torch
    from emurx import abi
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_pingtx needs a HIP device (there is no CPU path)"
    frames = n_req * count
    rx = RxPath(0, max_ns=16, max_clients=16, max_frames=frames, max_bytes=frames * 80)
    assert rx.pingtx_reserve(n_req) == 0
    for i in range(n_req):
        assert rx.pingtx_add(template(i), 42, i % 4) == (0, i)
    req = np.zeros(n_req, abi.PINGTX_REQ_DTYPE)
    req["id"], req["seq"], req["count"], req["ts"] = np.arange(n_req), 0xABCD, count, time.time_ns()
    return rx, req, frames


def windows(fn, a):
    import bench_ping as BP
    us = []
    for _ in range(a.windows + 1):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        us.append((time.perf_counter() - t0) * 1e6 / a.reps)
    return BP.stat(us[1:])


def slot_step(case, a):
    n_req, count = CASES[case]
    rx, req, frames = setup(n_req, count)
    for s in (0, 1):
        rx.egress_buffer(s)
    rx.egress_ping_buffer(0)[:n_req] = req

    def ping():
        assert rx.egress_submit_ping(0, 0, 0, n_req, 0) == 0
        return rx.egress_wait(0, copy=False)
    for _ in range(3):
        res = ping()
    assert res["n_frames"] == frames and res["n_msgs"] == frames // 64
    msgs = res["msgs"].copy()
    # the generated frames out of their messages (64 frames of 4 + 70 bytes behind 4), as a caller
    # of the plain path holds them: back to back
    m = msgs.reshape(frames // 64, 4 + 64 * 74)[:, 4:].reshape(frames, 74)
    vport = m[:, 1].copy()
    hf, hd = rx.egress_buffer(1)
    hf[:frames * 70] = m[:, 4:].reshape(-1)
    hd["off"][:frames], hd["len"][:frames], hd["vport"][:frames], hd["pad"][:frames] = np.arange(frames) * 70, 70, vport, 0

    def plain():
        rx.egress_submit(1, frames, frames * 70, 0)
        return rx.egress_wait(1, copy=False)
    for _ in range(3):
        pres = plain()
    assert pres["n_frames"] == frames and pres["msgs"].tobytes() == msgs.tobytes(), "the two paths' messages differ"
    out = {"requests": n_req, "count": count, "frames": frames, "msg_bytes": int(res["bytes"]),
           "h2d_bytes_per_frame": {"ping": round(16 * n_req / frames, 2), "plain": 78}}
    # alternating, so that a drift of the machine falls on both
    p1, q1 = windows(ping, a), windows(plain, a)
    p2, q2 = windows(ping, a), windows(plain, a)
    out["ping_slot_us"], out["plain_slot_us"] = (p1, p2), (q1, q2)
    pm, qm = min(p1["median"], p2["median"]), min(q1["median"], q2["median"])
    spread = max(q["max"] - q["min"] for q in (q1, q2))
    out["plain_minus_ping_us"] = round(qm - pm, 1)
    out["plain_window_spread_us"] = round(spread, 1)
    out["faster_beyond_plain_spread"] = bool(qm - pm > spread)
    out.update(reps=a.reps, windows=a.windows)
    rx.close()
    return out


def dev_step(a):
    import bench_ping as BP
    import torch
    from emurx import abi
    out = {}
    for case in ("a", "b"):
        n_req, count = CASES[case]
        rx, req, frames = setup(n_req, count)
        st = torch.cuda.current_stream()
        t_req = torch.from_numpy(req.view(np.uint8).copy()).to("cuda")
        S = [dict(out=torch.zeros(frames * 80 + 16, dtype=torch.uint8, device="cuda"),
                  desc=torch.zeros(frames * 8, dtype=torch.uint8, device="cuda"),
                  info=torch.zeros(abi.PTX_INFO_WORDS, dtype=torch.int64, device="cuda")) for _ in range(a.slots)]

        def call(s):
            assert rx.pingtx_dev(t_req, n_req, s["out"], frames * 80, s["desc"], frames, None, s["info"], stream=st.cuda_stream) == 0
        for s in S:
            call(s)
        torch.cuda.synchronize()
        assert S[0]["info"].cpu().numpy().tolist()[:6] == [frames, frames * 80, frames, n_req, 0, 0]
        us = []
        for _ in range(a.windows + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for r in range(a.reps):
                call(S[r % len(S)])
            e1.record(st)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        out[f"pingtx_dev_{case}_us"] = BP.stat(us[1:])
        rx.close()
    out.update(reps=a.reps, windows=a.windows, slots=a.slots)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--slots", type=int, default=2, help="copies of the outputs the timed device calls rotate over")
    ap.add_argument("--case", help="(child) run one step in this process")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pingtx" / "bench.json"), help="where the JSON line is written too")
    a = ap.parse_args()
    if a.case:
        sys.path.insert(0, str(ROOT / "trex-emu_amd"))
        sys.path.insert(0, str(Path(__file__).resolve().parent))
        print(json.dumps({"step": a.case, **(dev_step(a) if a.case == "c" else slot_step(a.case, a))}))
        return 0
    res = {"bench": "pingtx", "steps": []}
    for step in a.steps.split(","):
        print(f"step {step}", file=sys.stderr, flush=True)
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--case", step, "--reps", str(a.reps),
                            "--windows", str(a.windows), "--slots", str(a.slots)], stdout=subprocess.PIPE, text=True)
        if p.returncode:  # nothing more on the GPU after a failed step
            res["failed"] = {"step": step, "rc": p.returncode}
            break
        res["steps"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
