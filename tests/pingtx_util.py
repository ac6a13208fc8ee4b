"""Helpers of the ping send-side tests: templates, a mirror of the handle's template store, and
one emurx_pingtx_dev call compared with pingtx_ref.generate."""
import random
import struct

import numpy as np

import pingtx_ref as R
import sim_envs
from emurx import abi

NS_VLANS = struct.unpack_from("<II", sim_envs.NS_KEY, 4)
HUGE = 1 << 40


def capture_templates():
    """The templates of the two ping simulations (tests/test_pingtx_ref.py checks them against the
    captures): [(icmp_off, bytes)] for icmp3.json and ipv6ping_rpc.json."""
    e4, e6 = sim_envs.ENVS["icmp"], sim_envs.ENVS["ipv6"]
    o4, t4 = R.template4(e4["mac"], NS_VLANS, e4["ipv4"], bytes([16, 0, 0, 1]), R.SIM_IDENT, R.SIM_SEQ, payload_size=20)
    o6, t6 = R.template6(e6["mac"], NS_VLANS, e6["ipv6"], e6["ipv6"][:15] + b"\x01", R.SIM_IDENT, R.SIM_SEQ)
    return [(o4, bytes(t4)), (o6, bytes(t6))]


def capture_frames(z, capture, ids):
    return [z["data"][z["off"][i]:z["off"][i] + z["len"][i]].tobytes() for i in ids]


def raw_template(rng: random.Random, length: int, icmp_off: int, seq_t=None, ts_t=None) -> bytes:
    """`length` random bytes: the store and the generator read nothing but the three patched fields,
    so any bytes with a checksum field other than 0xffff are a template."""
    assert icmp_off + 24 <= length <= abi.PINGTX_MAX_LEN
    t = bytearray(rng.randrange(256) for _ in range(length))
    if seq_t is not None:
        struct.pack_into(">H", t, icmp_off + 6, seq_t)
    if ts_t is not None:
        struct.pack_into(">Q", t, icmp_off + 16, ts_t)
    if R.be16(t, icmp_off + 2) == 0xFFFF:
        t[icmp_off + 2] = 0x12
    return bytes(t)


class Store:
    """The handle's template store and its Python mirror, the dict pingtx_ref.generate takes."""

    def __init__(self, rx, max_pings):
        assert rx.pingtx_reserve(max_pings) == 0
        self.rx, self.max, self.m = rx, max_pings, {}

    def add(self, tmpl, icmp_off, vport=1):
        rc, i = self.rx.pingtx_add(tmpl, icmp_off, vport)
        assert rc == 0 and i not in self.m and i < self.max, (rc, i)
        self.m[i] = (bytes(tmpl), icmp_off, vport)
        return i

    def remove(self, i):
        assert self.rx.pingtx_remove(i) == 0
        del self.m[i]


def reqs_array(reqs):
    a = np.zeros(len(reqs), abi.PINGTX_REQ_DTYPE)
    for k, r in enumerate(reqs):
        a[k] = r
    return a


def check_frames(out, desc, want_frames, want_desc, tag=None):
    """The frames at their descriptors, byte for byte; the gaps between them are unspecified."""
    assert desc.tobytes() == want_desc.tobytes(), (tag, desc[:4], want_desc[:4])
    for j, f in enumerate(want_frames):
        o = int(desc["off"][j])
        assert o % 16 == 0
        got = out[o:o + len(f)].tobytes()
        assert got == f, (tag, j, got.hex(), f.hex())


class Call:
    """One emurx_pingtx_dev call, checked against generate(): frames, descriptors, outcomes and info,
    and the canaries behind out_cap and descriptor desc_cap.  out_cap / desc_cap None: exactly what
    the requests need.  The buffers are filled on torch's stream: synchronise before launch()."""

    def __init__(self, rx, mirror, reqs, out_cap=None, desc_cap=None, tag=None):
        import torch
        from gpu_util import to_dev
        need = R.generate(mirror, reqs, HUGE, HUGE)[3]
        self.out_cap = int(need[1]) if out_cap is None else out_cap
        self.desc_cap = int(need[2]) if desc_cap is None else desc_cap
        self.want = R.generate(mirror, reqs, self.out_cap, self.desc_cap)
        self.rx, self.n, self.tag = rx, len(reqs), tag
        self.t_req = to_dev(reqs_array(reqs))
        self.t_out = torch.full((self.out_cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t_desc = torch.full(((self.desc_cap + 4) * 8,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t_oc = torch.full((self.n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        self.t_info = torch.full((abi.PTX_INFO_WORDS + 2,), -1, dtype=torch.int64, device="cuda")

    def launch(self, stream=None):
        assert self.rx.pingtx_dev(self.t_req, self.n, self.t_out, self.out_cap, self.t_desc, self.desc_cap, self.t_oc,
                                  self.t_info, stream=stream) == 0, self.tag

    def finish(self):
        import torch
        torch.cuda.synchronize()
        tag, n, out_cap, desc_cap = self.tag, self.n, self.out_cap, self.desc_cap
        want_f, want_d, want_o, want_i = self.want
        out, oc = self.t_out.cpu().numpy(), self.t_oc.cpu().numpy()
        desc = self.t_desc.cpu().numpy().view(abi.DESC_DTYPE)
        info = self.t_info.cpu().numpy().view(np.uint64)
        assert info[:abi.PTX_INFO_WORDS].tolist() == want_i.tolist(), (tag, info, want_i)
        assert info[abi.PTX_INFO_WORDS] == (1 << 64) - 1
        assert oc[:n].tolist() == want_o.tolist(), tag
        assert (oc[n:] == 0xA5).all() and (out[out_cap:] == 0xA5).all(), tag
        assert (desc[desc_cap:].view(np.uint8) == 0xA5).all(), tag
        check_frames(out, desc[:len(want_f)], want_f, want_d, tag)
        return dict(frames=want_f, desc=want_d, outcome=want_o, info=want_i, out=out)


def run(rx, mirror, reqs, out_cap=None, desc_cap=None, stream=None, tag=None):
    import torch
    c = Call(rx, mirror, reqs, out_cap, desc_cap, tag)
    torch.cuda.synchronize()
    c.launch(stream)
    return c.finish()
