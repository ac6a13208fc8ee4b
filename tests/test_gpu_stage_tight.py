"""The tight 5 KiB staging slab of k_rx (7 workgroups per CU; EMURX_STAGE=tight, and the
launcher's automatic choice): bit-exact against the CPU oracle on records, queues and counters,
on both of its paths (a wave whose 16-byte-aligned byte range fits 320 vectors is staged, any
other takes the window path with an 80-byte window per lane), and the launcher's rule.

The last test needs no GPU: it compiles emurx_kernels.hip and reads the compiler's resource
report of the three classify instantiations.
"""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edge_frames as E
from emurx import abi
from emurx import frames as F
from emurx import synth
from gpu_util import frame_tuples, frames_tables, load_frame_tables, rec_diff, run_dev, to_dev
from test_gpu_parity import _dev_out, _spaced, check_batch, new_pair

gpu = pytest.mark.gpu
TIGHT = 5120


@pytest.fixture(scope="module")
def rxmod(gpu_ok, oracle_built):
    from emurx.rx import RxPath
    return RxPath


@pytest.fixture
def tight(monkeypatch):
    monkeypatch.setenv("EMURX_STAGE", "tight")  # read by emurx_open


def _loaded_pair(rxmod, w):
    rx, o = new_pair(rxmod)
    synth.load_tables(w, rx)
    synth.load_tables(w, o)
    return rx, o


# ---- forced tight: parity ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cfg,n", [("config_b", n) for n in (1, 63, 64, 65, 255, 256, 257, 4099)] +
                         [("config_c", 4096), ("config_e", 2048)])  # C and E: the window path
def test_tight_configs(rxmod, tight, cfg, n):
    w = getattr(synth, cfg)(n)
    rx, o = _loaded_pair(rxmod, w)
    check_batch(rx, o, w["buf"], w["desc"])
    assert rx.last_stage() == TIGHT


@gpu
@pytest.mark.parametrize("classify", [True, False])
def test_tight_edge_cases(rxmod, tight, classify):
    frames = [c[1] for c in E.cases()]
    rx, o = new_pair(rxmod)
    ns, cl = frames_tables(frames, vport=0)
    load_frame_tables([rx, o], ns, cl)
    buf, desc = F.pack_frames(frames, [c[2] for c in E.cases()])
    check_batch(rx, o, buf, desc, classify)
    assert rx.last_stage() == TIGHT


# ---- the staging boundary: 320 vectors are staged, 321 take the window path --------------------
@gpu
@pytest.mark.parametrize("mis", [1, 15])
def test_tight_staging_boundary(rxmod, tight, mis):
    """256 frames of 64 B, each wave in a 16 KiB region of its own.  Waves 0 and 3 are dense.
    Wave 1's first frame starts `mis` bytes past a 16-byte boundary and its last frame ends
    5,120 bytes past that boundary: 320 vectors, the largest staged range.  Wave 2's last frame
    ends one byte later: 321 vectors, the window path."""
    w = synth.config_b(256)
    d = w["desc"]
    off = np.zeros(256, np.int64)
    for wave in range(4):
        base, j = wave * 16384, np.arange(64)
        if wave in (1, 2):
            off[wave * 64:wave * 64 + 64] = base + mis + 80 * j
            off[wave * 64 + 63] = base + 320 * 16 + (wave == 2) - 64
        else:
            off[wave * 64:wave * 64 + 64] = base + 4 + 68 * j
    for wave, want in ((1, 320), (2, 321)):
        o_ = off[wave * 64:wave * 64 + 64]
        assert (np.diff(o_) >= 64).all()
        assert -(-(o_[-1] + 64 - (o_[0] & ~15)) // 16) == want
    buf = np.zeros(4 * 16384 + 64, np.uint8)
    nd = d.copy()
    for i in range(256):
        s, n = int(d["off"][i]), int(d["len"][i])
        buf[off[i]:off[i] + n] = w["buf"][s:s + n]
    nd["off"] = off.astype(np.uint32)
    rx, o = _loaded_pair(rxmod, w)
    rec = check_batch(rx, o, buf, nd)
    assert (rec["status"] == 0).all() and (rec["client_id"] == 0).all()
    assert rx.last_stage() == TIGHT


# ---- the 80-byte window edge -----------------------------------------------------------------
def _edge_window_frames():
    """Frames whose L4 header starts at frame byte 78 (two tags, IPv6, two 8-byte extension
    headers) or 82 (one tag, IPv6, three), as udp, tcp and an ICMPv6 echo request.  The window
    of a lane starts at its frame's 16-byte boundary, so a frame at address = head mod 16 has
    its L4 header at window byte head + 78: with head 0, 2 and 4 it starts at window byte 78,
    80 and 82, below, on and past the 80-byte edge (head 15: the IPv6 destination crosses it
    too).  Every frame comes intact and with the byte on either side of the edge corrupted."""
    pad = bytes([1, 4, 0, 0, 0, 0])
    out = []
    for l4 in (78, 82):
        nx = 2 if l4 == 78 else 3
        for proto in ("udp", "tcp", "echo"):
            nh = {"udp": 17, "tcp": 6, "echo": 58}[proto]
            exts = b"".join(F.ipv6_ext(60 if k + 1 < nx else nh, pad) for k in range(nx))
            if proto == "udp":
                body = F.udp(4000, 5000, b"window-edge!", csum="auto", pseudo=E.ph6(20, 17))
            elif proto == "tcp":
                body = F.tcp(1000, 80, b"window-edge!", csum="auto", pseudo=E.ph6(32, 6))
            else:
                body = F.icmp6(128, 0, b"\x00\x01\x00\x01edge", pseudo=E.ph6(12, 58))
            ip = F.ipv6(E.SIP6, E.DIP6, 0, exts + body)
            tags = (F.dot1q(5, F.ETH_DOT1Q) + F.dot1q(6, F.ETH_IPV6)) if l4 == 78 else F.dot1q(7, F.ETH_IPV6)
            f = F.ethernet(E.D, E.S, F.ETH_QINQ if l4 == 78 else F.ETH_DOT1Q, tags + ip)
            assert f[l4 - 8] == nh and len(f) > l4 + 8
            for head in (0, 2, 4, 15):
                for bad in (None, 79 - head, 80 - head):
                    g = bytearray(f)
                    if bad is not None:
                        g[bad] ^= 0xFF
                    out.append((bytes(g), head))
    return out


@gpu
def test_tight_window_edge(rxmod, tight):
    """Waves on the window path (frames 128 B apart: 8 KiB per wave) whose headers cross the
    80-byte window edge: records (statuses among them), queues and counters equal the oracle's."""
    cases = _edge_window_frames()
    cases = (cases * 2)[:128]  # two full waves: a short last wave would fit the slab
    frames = [c[0] for c in cases]
    rx, o = new_pair(rxmod)
    ns, cl = frames_tables(frames, vport=0)
    load_frame_tables([rx, o], ns, cl)
    buf = np.zeros(len(cases) * 128 + 256, np.uint8)
    desc = np.zeros(len(cases), abi.DESC_DTYPE)
    for i, (f, head) in enumerate(cases):
        at = i * 128 + head
        buf[at:at + len(f)] = np.frombuffer(f, np.uint8)
        desc[i]["off"], desc[i]["len"] = at, len(f)
    rec = check_batch(rx, o, buf, desc)
    st = rec["status"]
    assert (st == 0).sum() >= len(cases) // 3  # the intact frames at least
    for name in ("UDP_CS", "TCP_CS", "ICMPV6_CS"):
        assert (st == abi.ST[name]).any(), name
    assert ((rec["flags"] >> 4) & 7 == abi.LK["CLIENT"]).any()
    assert rx.last_stage() == TIGHT


# ---- transport flows: the tuple is read behind the lookups, from the parked fields ------------
@gpu
@pytest.mark.parametrize("cfg,n", [("config_b", 4099), ("config_c", 6000)])  # staged; mostly window
def test_tight_flows(rxmod, tight, cfg, n):
    w = synth.config_b(n) if cfg == "config_b" else synth.config_c(n, syn=0.3)
    rx, o = _loaded_pair(rxmod, w)
    buf, desc = w["buf"], w["desc"]
    orec = o.rx_batch(buf, desc)[0]
    tup = frame_tuples(buf, desc, orec)
    idx = np.array([i for i, t in enumerate(tup) if t is not None])
    assert len(idx) > n // 2
    rng = np.random.default_rng(7)
    for c in np.unique(orec["client_id"][idx])[::2]:
        assert rx.client_set_transport(int(c), 1) == o.client_set_transport(int(c), 1) == 0
    for i in rng.choice(idx, len(idx) // 3, replace=False):
        cid = int(orec[i]["client_id"])
        assert rx.flow_add(cid, tup[i], int(i)) == o.flow_add(cid, tup[i], int(i))
    rec, _, _, _, flow = run_dev(rx, buf, desc, flows=True)
    orec = o.rx_batch(buf, desc)[0]
    assert rec.tobytes() == orec.tobytes(), rec_diff(rec, orec)
    want = o.flows(buf, desc, orec)
    assert np.array_equal(flow, want)
    assert (want <= abi.FLOW_ID_MAX).sum() > 100
    assert rx.last_stage() == TIGHT


# ---- the automatic choice ---------------------------------------------------------------------
def _run_seq(rx, o, batches):
    """last_stage() after each launch; every launch's outputs against the oracle's (computed
    once per distinct batch)."""
    from emurx.rx import hist_to_counters
    import pyoracle
    want, seq = {}, []
    for buf, desc in batches:
        if id(buf) not in want:
            orec, oq, oqoff, ocnt = o.rx_batch(buf, desc)
            want[id(buf)] = (orec.tobytes(), oq, oqoff, pyoracle.counters_dict(ocnt))
        orec, oq, oqoff, ocnt = want[id(buf)]
        rec, qlist, qoff, hist = run_dev(rx, buf, desc)
        assert rec.tobytes() == orec and np.array_equal(qlist, oq) and np.array_equal(qoff, oqoff)
        got = hist_to_counters(hist)
        assert all(got[k] == ocnt[k] for k in abi.PARSER_COUNTER_NAMES)
        seq.append(rx.last_stage())
    return seq


@gpu
@pytest.mark.parametrize("stride,back", [(90, 6144), (100, 7168)])
def test_tight_auto_choice(rxmod, monkeypatch, stride, back):
    """Launches 1, 9, 17, 25 copy their samples back and, every batch being synchronised,
    launches 2, 10, 18, 26 decide.  Dense 64-byte frames: launch 2 sees the tight slab eligible
    and takes the narrow one, launch 10 sees it eligible again and takes it.  Launch 18 decides
    from launch 17's dense sample, so the spaced frames (5,760 or 6,400 B per wave: over 5 KiB)
    first run on the tight slab's window path; launch 26 sees them and leaves at once, to the
    narrow slab or, for the 6-7 KiB band, the wide one.  Dense again: launch 34 still decides
    from launch 33's spaced sample; launch 42, the first to see a dense one, takes the narrow
    slab, not the tight one."""
    monkeypatch.delenv("EMURX_STAGE", raising=False)
    w = synth.config_b(1 << 16)
    rx, o = _loaded_pair(rxmod, w)
    dense = (w["buf"], w["desc"])
    spaced = _spaced(w, stride)
    seq = _run_seq(rx, o, [dense] * 17 + [spaced] * 16 + [dense] * 9)
    assert seq == [7168] + [6144] * 8 + [5120] * 16 + [back] * 16 + [6144], seq


# ---- the routed kinds -------------------------------------------------------------------------
@gpu
def test_tight_routed_kinds(rxmod, tight):
    """classify_route_dev (kind 1 with the owner counts) and parse_route_dev + lookup_dev
    (kind 2) on the tight slab: every kind has a 5 KiB instantiation, so that is what ran."""
    import torch
    import route_ref
    from emurx import exchange as X
    from test_gpu_tables import tail_cap_max
    n, parts, me = 20000 + 77, 2, 1
    w = synth.config_c(n, rank=me)
    rx, o = _loaded_pair(rxmod, w)
    orec = o.rx_batch(w["buf"], w["desc"])[0]
    buf, desc = to_dev(w["buf"]), to_dev(w["desc"])
    cap = X.capacity(n, parts)
    d = _dev_out(n)
    send = torch.full((parts * cap * X.REC_BYTES,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((parts,), -1, dtype=torch.int32, device="cuda")
    rx.classify_route_dev(buf, desc, n, d["rec"], d["qlist"], d["qcap"], d["tile_cnt"], d["hist"], parts, me, cap,
                          send, cnt)
    torch.cuda.synchronize()
    assert rx.last_stage() == TIGHT
    assert d["rec"].cpu().numpy()[: n * 32].view(abi.REC_DTYPE).tobytes() == orec.tobytes()
    want = route_ref.route(orec, parts, me)
    c = cnt.cpu().numpy()
    assert list(c) == [len(x) for x in want]
    sreg = send.cpu().numpy().view(abi.ROUTE_REC_DTYPE).reshape(parts, cap)
    for k in range(parts):
        assert sreg[k, : c[k]].tobytes() == want[k].tobytes(), k
    # kind 2: one partition, the owner's lookups give the oracle's records in frame order
    src = rxmod(0, max_ns=4096, max_clients=65536, max_frames=n)
    src.register_all()
    synth.load_tables(w, src)
    cap, tcap = n, tail_cap_max(n)
    d = _dev_out(n)
    sd = torch.full((abi.lookup_region_bytes(cap, tcap),), 0xEE, dtype=torch.uint8, device="cuda")
    sc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    src.parse_route_dev(buf, desc, n, None, d["qlist"], d["qcap"], d["tile_cnt"], d["hist"], 1, 0, cap, sd, sc,
                        tail_cap=tcap)
    torch.cuda.synchronize()
    assert src.last_stage() == TIGHT
    out = torch.full((cap * X.REC_BYTES,), 0xEE, dtype=torch.uint8, device="cuda")
    src.lookup_dev(sd, sc, 1, cap, out, tail_cap=tcap)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(abi.ROUTE_REC_DTYPE)[:n]
    assert list(sc.cpu().numpy()) == [n, 0]
    assert got["rec"].tobytes() == orec.tobytes(), rec_diff(got["rec"], orec)


# ---- not GPU: the compiler's resource report ---------------------------------------------------
def test_k_rx_resources():
    """k_rx<1, 5120> fits 7 waves per SIMD without scratch; the 6 KiB and 7 KiB builds keep 6
    and 5 without scratch (hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags)."""
    pkg = Path(__file__).resolve().parent.parent / "trex-emu_amd"
    mk = (pkg / "Makefile").read_text()
    hipcc = re.search(r"^HIPCC \?= (.*)$", mk, re.M).group(1).strip()
    if not (Path(hipcc).exists() or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    arch = re.search(r"^ARCH \?= (.*)$", mk, re.M).group(1).strip()
    flags = re.search(r"^HIPFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()
    p = subprocess.run([hipcc, *flags, "--offload-device-only", "-c", "csrc/emurx_kernels.hip", "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], cwd=pkg, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    res = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", p.stderr, re.S):
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", body)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", body)
        if scratch and occ:
            res[name] = (int(scratch.group(1)), int(occ.group(1)))
    for stage, occ in ((5120, 7), (6144, 6), (7168, 5)):
        name = f"_ZN5emurx4k_rxILi1ELj{stage}EEEvNS_6RxArgsE"  # emurx::k_rx<1, stage>(RxArgs)
        assert res.get(name) == (0, occ), (stage, res.get(name))
