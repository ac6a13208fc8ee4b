#!/usr/bin/env python3
"""Measure the ping fold (emurx_ping_dev, emurx_ingest_set_ping) and what it must not slow down,
and print one JSON line.

Steps, each a GPU step of its own (a child process under `timeout`; a failing step ends the run,
nothing more is started on the GPU after it):
  none   a --n frame config-C batch with no ICMP at all (the descriptors of its ICMPv4 / ICMPv6
         frames point at one of its UDP frames): emurx_ping_dev beside emurx_learn_dev on the same
         batch and records: both read half a record per frame and find no candidate.
  real   the same batch with 1 % of its frames replaced by ICMPv4 echo replies to 10,000 distinct
         clients, one reply per key: the realistic case.
  twice  `real` with sixteen of its keys seen twice, spread over the batch: the ordered pass runs,
         over the steps that hold such a reply.
  flood  --n echo replies of one ping (ascending sequence numbers): the ordered pass's worst case.
  slot   an ingest slot at 65,536 frames (`real` at that size, as messages of 64 frames), every
         answer kind on, with ping on against ping off: submit -> wait per batch.
  base   what shares no hot code with the fold, with --parent DIR (a tree of the parent commit with
         its library built: DIR/emurx, DIR/lib/libemurx.so) for this tree and the parent,
         alternating, --rounds times each: emurx_learn_dev and emurx_nsstat_dev on bench_respond's
         case c at --n frames, and the ingest slot of `slot` with answers on and ping off.
  bench  with --parent: bench.py --gpus 1 --config B and C, --bench-repeats times for each tree,
         alternating (the parent's library through EMURX_LIB).

Device calls are timed between one HIP event pair, rotating over --slots copies of the batch, the
mean per call of a window of --reps calls after two warm-up rotations; ingest times are a host
clock around submit .. wait.  Every figure is the median of --windows windows (behind one more that is
dropped: it still warms up) with the smallest and largest beside it, in microseconds.  Against the parent the bar is the parent's own spread
(largest minus smallest window, or run, over at least five).

    python tools/bench_ping.py [--steps none,real,twice,flood,slot,base,bench] [--parent DIR] [--out profiles/ping/bench.json]
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
NOW = 1_700_000_000_123_456_789
MAGIC = 0xC15C0C15C0BE5BE5


def stat(a):
    a = np.array(a, dtype=np.float64)
    return {"median": round(float(np.median(a)), 1), "min": round(float(a.min()), 1), "max": round(float(a.max()), 1)}


def echo_reply(mac, ip4, key, ident, seq, ts):
    """An ICMPv4 echo reply to the client, 24 bytes of ICMP and a 2-byte word that keeps the
    checksum the same for every sequence number."""
    import bench_respond as BR
    from emurx import frames as F
    pay = MAGIC.to_bytes(8, "big") + ts.to_bytes(8, "big") + (0xFFFF - (seq & 0xFFFF)).to_bytes(2, "big")
    ip = F.ipv4(bytes([48, 0, 0, 9]), bytes(ip4), 1, F.icmp4(0, 0, ident, seq & 0xFFFF, pay))
    return bytes(mac) + BR.DUT + BR._tags(key) + b"\x08\x00" + ip


def batch_none(n):
    """Config C without ICMP: the descriptors of its ICMP frames point at its first UDP frame."""
    import pyoracle
    from emurx import abi, synth
    w = synth.config_c(n)
    o = pyoracle.Oracle()
    synth.load_tables(w, o)
    rec, _, _, _ = o.rx_batch(w["buf"], w["desc"])
    icmp = (rec["proto"] == abi.CB_ICMP) | (rec["proto"] == abi.CB_ICMPV6)
    udp = int(np.nonzero((rec["proto"] == abi.CB_UDP) & (rec["status"] == 0))[0][0])
    w["desc"] = w["desc"].copy()
    w["desc"][icmp] = w["desc"][udp]
    w.update(name="C, no ICMP", replaced=int(icmp.sum()))
    return w


def batch_real(n, share=0.01, clients=10000, seed=5):
    """batch_none with `share` of the frames replaced by echo replies to `clients` distinct clients
    (every one its own key: one reply per key while share * n <= clients)."""
    import struct
    w = batch_none(n)
    rng = np.random.default_rng(seed)
    k = int(n * share)
    c = w["clients"]
    idx = np.sort(rng.choice(n, k, replace=False))
    pick = rng.choice(len(c["cid"]), min(max(clients, k), len(c["cid"])), replace=False)
    keys = {ns_id: key for key, ns_id in w["ns"]}
    extra, base = bytearray(), (len(w["buf"]) + 63) & ~63
    for j, i in enumerate(idx):
        cl = int(pick[j % len(pick)])
        key = keys[int(c["ns"][cl])]
        f = echo_reply(c["mac"][cl].tobytes(), c["ipv4"][cl].tobytes(), key, 0x1234, 0xABCD + j // len(pick), NOW - 1_000_000 - j)
        extra += bytes(4)
        w["desc"][i]["off"], w["desc"][i]["len"], w["desc"][i]["vport"] = base + len(extra), len(f), struct.unpack("<H", key[:2])[0]
        extra += f
    buf = np.zeros(base + len(extra) + 64, np.uint8)
    buf[: len(w["buf"])] = w["buf"]
    buf[base: base + len(extra)] = np.frombuffer(bytes(extra), np.uint8)
    w.update(name=f"C, no ICMP + {share:.0%} echo replies", buf=buf, replies=k, reply_idx=idx)
    return w


def batch_twice(n, keys=16):
    """batch_real with the replies of `keys` of its pings repeated (the next sequence number, in a
    slot of a UDP frame far behind the first): a few keys with two accepted replies."""
    w = batch_real(n)
    d = w["desc"]
    rep = w["reply_idx"]
    src = rep[:: max(len(rep) // keys, 1)][:keys]
    seen = set(rep.tolist())
    extra, base = bytearray(), (len(w["buf"]) + 63) & ~63
    for i in src:
        f = bytearray(np.asarray(w["buf"])[int(d["off"][i]): int(d["off"][i]) + int(d["len"][i])].tobytes())
        at = len(f) - 26  # the ICMP header of echo_reply's frame: sequence number + 1, the balancing word - 1
        seq = ((f[at + 6] << 8 | f[at + 7]) + 1) & 0xFFFF
        f[at + 6], f[at + 7] = seq >> 8, seq & 0xFF
        f[at + 24], f[at + 25] = (0xFFFF - seq) >> 8, (0xFFFF - seq) & 0xFF
        j = (int(i) + len(d) // 2) % len(d)
        while j in seen:
            j = (j + 1) % len(d)
        seen.add(j)
        extra += bytes(4)
        d[j]["off"], d[j]["len"], d[j]["vport"] = base + len(extra), len(f), d[i]["vport"]
        extra += f
    buf = np.zeros(base + len(extra) + 64, np.uint8)
    buf[: len(w["buf"])] = w["buf"]
    buf[base: base + len(extra)] = np.frombuffer(bytes(extra), np.uint8)
    w.update(name=w["name"] + f", {keys} keys twice", buf=buf)
    return w


def batch_flood(n):
    """n echo replies of one ping to the one client of an untagged Namespace, sequence numbers
    counting up (the checksum stays: echo_reply's balancing word)."""
    from emurx import abi, frames as F
    key = F.tunnel_key(0, 0, 0)
    mac, ip = bytes([0, 0, 1, 0, 0, 0]), bytes([16, 1, 0, 0])
    tmpl = np.frombuffer(echo_reply(mac, ip, key, 0x1234, 0, NOW - 1000), np.uint8)
    fr = np.tile(tmpl, (n, 1))
    seq = (np.arange(n) & 0xFFFF).astype(np.uint32)
    at = 14 + 20  # the ICMP header
    fr[:, at + 6], fr[:, at + 7] = seq >> 8, seq & 0xFF
    fr[:, at + 24], fr[:, at + 25] = (0xFFFF - seq) >> 8, (0xFFFF - seq) & 0xFF
    stride = 64
    buf = np.zeros(n * stride + 64, np.uint8)
    buf[: n * stride].reshape(n, stride)[:, : fr.shape[1]] = fr
    desc = np.zeros(n, abi.DESC_DTYPE)
    desc["off"], desc["len"] = np.arange(n, dtype=np.uint32) * stride, fr.shape[1]
    cl = dict(ns=np.zeros(1, np.int64), cid=np.arange(1), mac=np.frombuffer(mac, np.uint8).reshape(1, 6).copy(),
              ipv4=np.frombuffer(ip, np.uint8).reshape(1, 4).copy(), ipv6=np.zeros((1, 16), np.uint8))
    return dict(name="one ping", buf=buf, desc=desc, n=n, ns=[(key, 0)], clients=cl)


def repack(w):
    """w's frames gathered into the ZMQ layout in descriptor order (each frame behind its 4-byte
    frame header, back to back): what emurx.frames.zmq_messages cuts into messages."""
    d = w["desc"]
    ln, src = d["len"].astype(np.int64), d["off"].astype(np.int64)
    off = np.cumsum(ln + 4) - ln
    buf = np.zeros(int(off[-1] + ln[-1]) + 64, np.uint8)
    buf[off - 4], buf[off - 3], buf[off - 2], buf[off - 1] = 0xAA, d["vport"], ln >> 8, ln & 0xFF
    k = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)  # byte index inside its frame
    buf[np.repeat(off, ln) + k] = np.asarray(w["buf"])[np.repeat(src, ln) + k]
    desc = d.copy()
    desc["off"] = off
    return dict(w, buf=buf, desc=desc)


class Dev:
    """A batch on the device, --slots copies at distinct addresses, classified; timed windows."""

    def __init__(self, w, slots, reps, windows):
        import torch
        from emurx import abi, synth
        from emurx.rx import RxPath
        assert torch.cuda.is_available(), "bench_ping needs a HIP device (there is no CPU path)"
        self.torch, self.abi, self.reps, self.windows = torch, abi, reps, windows
        self.n = n = len(w["desc"])
        self.rx = RxPath(0, max_ns=4096, max_clients=1 << 17, max_frames=n)
        self.rx.register_all()
        synth.load_tables(w, self.rx)
        self.st = torch.cuda.current_stream()

        def dev(a, pad=64):
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            t = torch.zeros(b.size + pad, dtype=torch.uint8, device="cuda")
            t[: b.size] = torch.from_numpy(b.copy()).to("cuda")
            return t
        hist = torch.zeros(abi.HIST_SHARDS * 2 * abi.HIST_BINS, dtype=torch.int64, device="cuda")
        self.S = []
        for _ in range(slots):
            s = dict(buf=dev(w["buf"]), desc=dev(w["desc"]), rec=torch.zeros(n * 32, dtype=torch.uint8, device="cuda"),
                     oc=torch.empty(n, dtype=torch.uint8, device="cuda"), oc2=torch.empty(n, dtype=torch.uint8, device="cuda"),
                     oc3=torch.empty(n, dtype=torch.uint8, device="cuda"), info=torch.zeros(16, dtype=torch.int64, device="cuda"))
            self.rx.classify_dev(s["buf"], s["desc"], n, s["rec"], None, 0, None, hist, stream=self.st.cuda_stream)
            self.S.append(s)
        torch.cuda.synchronize()

    def window(self, fn):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.st)
        for k in range(self.reps):
            fn(self.S[k % len(self.S)])
        e1.record(self.st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / self.reps  # us per call

    def timed(self, fns):
        """{name: fn(slot)} -> {name: stat}, the windows taken in turn."""
        for fn in fns.values():
            for _ in range(2):
                for s in self.S:
                    fn(s)
        us = {k: [] for k in fns}
        for _ in range(self.windows + 1):
            for k, fn in fns.items():
                us[k].append(self.window(fn))
        return {k: stat(v[1:]) for k, v in us.items()}  # the first window of each still warms up: dropped

    def learn_fn(self):
        """emurx_learn_dev with room for its keys (sized by a call with room for one)."""
        torch, rx, n, st = self.torch, self.rx, self.n, self.st
        s0 = self.S[0]
        one = torch.empty(40, dtype=torch.uint8, device="cuda")
        rx.learn_dev(s0["buf"], s0["desc"], s0["rec"], n, one, 1, s0["oc2"], s0["info"], stream=st.cuda_stream)
        torch.cuda.synchronize()
        cap = max(int(s0["info"].cpu().numpy()[1]), 1)
        for s in self.S:
            s["lev"] = torch.empty(cap * 40, dtype=torch.uint8, device="cuda")
        return lambda s: rx.learn_dev(s["buf"], s["desc"], s["rec"], n, s["lev"], cap, s["oc2"], s["info"], stream=st.cuda_stream)


def ping_step(w, a):
    """emurx_ping_dev beside emurx_learn_dev on w."""
    d = Dev(w, a.slots, a.reps, a.windows)
    torch, rx, n, st, abi = d.torch, d.rx, d.n, d.st, d.abi
    s0 = d.S[0]
    one = torch.empty(80, dtype=torch.uint8, device="cuda")
    rx.ping_dev(s0["buf"], s0["desc"], s0["rec"], n, NOW, one, 1, s0["oc"], s0["info"], stream=st.cuda_stream)
    torch.cuda.synchronize()
    cap = max(int(s0["info"].cpu().numpy()[1]), 1)
    for s in d.S:
        s["pev"] = torch.empty(cap * 80, dtype=torch.uint8, device="cuda")
    ping = lambda s: rx.ping_dev(s["buf"], s["desc"], s["rec"], n, NOW, s["pev"], cap, s["oc"], s["info"], stream=st.cuda_stream)  # noqa: E731
    t = d.timed({"ping_us": ping, "learn_us": d.learn_fn()})
    ping(s0)
    torch.cuda.synchronize()
    info = s0["info"].cpu().numpy().view(np.uint64)[: abi.PNG_INFO_WORDS]
    ev = s0["pev"].cpu().numpy()[: int(info[0]) * 80].view(abi.PING_EV_DTYPE)
    out = {"name": w["name"], "frames": n, "events": int(info[0]), "overflow": int(info[2]), "outcomes_1_5": [int(x) for x in info[3:8]],
           "n_ok": int(ev["n_ok"].sum()), "n_succ": int(ev["n_succ"].sum()), **t,
           "ping_over_learn": round(t["ping_us"]["median"] / t["learn_us"]["median"], 3), "reps": a.reps, "slots": a.slots,
           "windows": a.windows}
    rx.close()
    return out


def slot_step(w, kinds, fams, reps, windows):
    """submit -> wait of w's frames as 64-frame messages on slot 0."""
    import torch
    from emurx import frames as F, synth
    from emurx.rx import RxPath
    assert torch.cuda.is_available(), "bench_ping needs a HIP device (there is no CPU path)"
    w = repack(w)
    zs, msgs = F.zmq_messages(w["buf"], w["desc"], 64)
    n = len(w["desc"])
    rx = RxPath(0, max_ns=4096, max_clients=1 << 17, max_frames=n, max_bytes=len(zs) + 64)
    rx.register_all()
    synth.load_tables(w, rx)
    rx.ingest_set_answers(0, kinds)
    if fams:
        rx.ingest_set_ping(0, fams)
        rx.ingest_set_now(0, NOW)
    np.copyto(rx.ingest_buffer(0, len(zs)), zs)

    def batch():
        rx.ingest_submit(0, msgs)
        return rx.ingest_wait(0, copy=False)
    for _ in range(3):
        res = batch()
    assert res["n"] == n and not res["one_launch"]
    us = []
    for _ in range(windows + 1):
        t0 = time.perf_counter()
        for _ in range(reps):
            batch()
        us.append((time.perf_counter() - t0) * 1e6 / reps)
    us = us[1:]  # the first window still warms up: dropped
    out = {"frames": n, "msgs": len(msgs), "ping": fams, "us_per_batch": stat(us), "reps": reps, "windows": windows}
    if fams:
        p = rx.ingest_ping(0, n)
        out.update(events=len(p["ev"]), outcomes_1_5=[int(x) for x in p["info"][3:8]])
    rx.close()
    return out


def base_step(a):
    """What the fold shares no hot code with: learn and nsstat on bench_respond's case c, the ingest
    slot with answers on (and ping off), on whichever tree --pkg names."""
    import bench_respond as BR
    from emurx import abi
    d = Dev(BR.case_c(a.n), a.slots, a.reps, a.windows)
    torch, rx, n, st = d.torch, d.rx, d.n, d.st
    ncap = rx.nsstat_max_events()
    for s in d.S:
        s["odesc"] = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
        s["osrc"] = torch.empty(n, dtype=torch.int32, device="cuda")
        s["nev"] = torch.empty(ncap * 96, dtype=torch.uint8, device="cuda")
        rx.respond_dev(s["buf"], s["desc"], s["rec"], n, None, 0, s["odesc"], s["osrc"], s["oc"], s["info"], stream=st.cuda_stream,
                       kinds=abi.RSPK_ALL)
    learn = d.learn_fn()
    for s in d.S:
        learn(s)  # the learn outcomes nsstat reads
    nss = lambda s: rx.nsstat_dev(s["buf"], s["desc"], s["rec"], n, s["oc"], s["oc2"], s["nev"], ncap, s["oc3"], s["info"],  # noqa: E731
                                  kinds=abi.RSPK_ALL, stream=st.cuda_stream)
    out = d.timed({"learn_us": learn, "nsstat_us": nss})
    rx.close()
    del d
    out["ingest_answers_64k_us"] = slot_step(batch_real(1 << 16), abi.RSPK_ALL, 0, a.reps, a.windows)["us_per_batch"]
    return out


def run_child(a):
    sys.path.insert(0, str(Path(a.pkg).resolve()))
    sys.path.insert(0, str(ROOT / "oracle"))
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from emurx import abi
    if a.case == "none":
        return {"step": "none", **ping_step(batch_none(a.n), a)}
    if a.case == "real":
        return {"step": "real", **ping_step(batch_real(a.n), a)}
    if a.case == "twice":
        return {"step": "twice", **ping_step(batch_twice(a.n), a)}
    if a.case == "flood":
        return {"step": "flood", **ping_step(batch_flood(a.n), a)}
    if a.case == "slot":
        w = batch_real(1 << 16)
        return {"step": "slot", "name": w["name"], "off": slot_step(w, abi.RSPK_ALL, 0, a.reps, a.windows),
                "on": slot_step(w, abi.RSPK_ALL, abi.PNGK_ALL, a.reps, a.windows)}
    return {"step": "base", **base_step(a)}


def versus(parent, this):
    """parent, this: the figures of the runs of each tree -> the verdict against the parent's spread."""
    spread = max(parent) - min(parent)
    diff = float(np.median(this) - np.median(parent))
    return {"parent": parent, "this": this, "parent_spread": round(spread, 2), "this_minus_parent": round(diff, 2),
            "within_parent_spread": bool(abs(diff) <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="none,real,twice,flood,slot,base,bench")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--slots", type=int, default=4, help="copies of the batch the timed calls rotate over")
    ap.add_argument("--rounds", type=int, default=2, help="with --parent: runs of the base step per tree, alternating")
    ap.add_argument("--bench-repeats", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=50)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--parent", help="a tree of the parent commit, built (DIR/emurx, DIR/lib/libemurx.so)")
    ap.add_argument("--case", help="(child) run one step in this process")
    ap.add_argument("--pkg", default=str(ROOT / "trex-emu_amd"), help="(child) the tree emurx is imported from")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ping" / "bench.json"), help="where the JSON line is written too")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_child(a)))
        return 0

    def child(case, pkg):
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--case", case, "--pkg", pkg,
                            "--n", str(a.n), "--reps", str(a.reps), "--windows", str(a.windows), "--slots", str(a.slots)],
                           stdout=subprocess.PIPE, text=True)
        return json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else p.returncode

    def bench(config, lib):
        env = dict(os.environ)
        if lib:
            env["EMURX_LIB"] = lib
        p = subprocess.run(["timeout", "-k", "10", str(a.step_timeout), sys.executable, str(ROOT / "bench.py"), "--gpus", "1",
                            "--config", config, "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)],
                           stdout=subprocess.PIPE, text=True, env=env)
        return json.loads(p.stdout.strip().splitlines()[-1])["value"] if p.returncode == 0 else -p.returncode - 1000

    res = {"bench": "ping", "n": a.n, "steps": []}
    for step in a.steps.split(","):
        print(f"step {step}", file=sys.stderr, flush=True)
        if step == "bench" and not a.parent:  # this tree against the parent only
            continue
        if step in ("none", "real", "twice", "flood", "slot"):
            r = child(step, a.pkg)
        elif step == "base":
            trees = [("this", a.pkg)] + ([("parent", a.parent)] if a.parent else [])
            runs = {t: [] for t, _ in trees}
            r = None
            for _ in range(a.rounds if a.parent else 1):
                for t, pkg in reversed(trees):
                    x = child("base", pkg)
                    if isinstance(x, int):
                        r = x
                        break
                    runs[t].append(x)
                if r is not None:
                    break
            if r is None:
                r = {"step": "base", "runs": runs}
                if a.parent:  # every window of every run: the parent's spread over 2 * windows figures
                    for k in ("learn_us", "nsstat_us", "ingest_answers_64k_us"):
                        r[k] = versus([x[k][f] for x in runs["parent"] for f in ("min", "median", "max")],
                                      [x[k][f] for x in runs["this"] for f in ("min", "median", "max")])
        else:
            r = {"step": "bench", "unit": "Mpkt/s", "steps": a.bench_steps, "warmup": a.bench_warmup}
            for config in ("B", "C"):
                vals = {"parent": [], "this": []}
                for _ in range(a.bench_repeats):
                    for t, lib in (("parent", str(Path(a.parent) / "lib" / "libemurx.so")), ("this", None)):
                        vals[t].append(bench(config, lib))
                if min(vals["parent"] + vals["this"]) < 0:
                    r = 1
                    break
                r[config] = versus(vals["parent"], vals["this"])
        if isinstance(r, int):  # nothing more on the GPU after a failed step
            res["failed"] = {"step": step, "rc": r}
            break
        res["steps"].append(r)
    line = json.dumps(res)
    print(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
