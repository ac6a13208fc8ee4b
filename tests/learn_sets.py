"""Batches that put chosen keys at chosen places of the two hash sets of emurx_learn_dev's decide
pass (trex-emu_amd/csrc/emurx_learn.hip), so that the probe sequences of both sets are reached by
construction and not by luck.

The hash and the two start-slot rules are restated here (key_hash, lds_start, slots_of;
tests/test_learn_sets.py holds them against emurx_learn_key_hash).  Seeded sender addresses are
searched for keys that meet a condition:

    ARP requests and replies   24 bits of sender id in the IP (48.a.b.c) and 24 in the MAC
                               (00:10:94:a:b:c), in respond_ref's Namespaces (vport 1)
    solicitations              32 free bits at the end of a global source 2001:db8:ee::/96, the
                               source link-layer address fixed; nd_ref's Namespaces (vport 2)
    advertisements             32 free bits at the end of a global target 2001:db8:ef::/96 (bytes
                               11 and 12 are not ff:fe, so the target is no EUI-64 address)

Workgroup set (512 slots in LDS, start (h >> 9) & 511, used by a tile with 2 * leaders <= learners,
leaders = the sum over its four waves of the wave's distinct keys):
    L1  two different keys with equal start, led from different waves of one tile
    L2  two keys that start at slot 511 (and one at slot 0) led in one tile: the chain wraps
    L3  one key led by all four waves of a tile that is also in a second tile
    L4  the switch: tiles with (leaders, learners) = (128, 256), (129, 256), (1, 2) as a full tile;
        a ragged last tile cannot hold 256 learners, so there the same boundary is taken at 254:
        (127, 254) folds as 2 * 127 == 254, (128, 254) does not, and (1, 2) is a tile of two frames
    L5  at least 100 distinct keys in one folding tile, several of them displaced from their start
Global set (slots_of(n) slots, start h & mask, the owner word tagged with h >> 27):
    G1  two different keys with equal start and different tags
    G2  two different keys with equal start and equal tags: an ARP pair, an ND pair, and a pair that
        differs only in the MAC
    G3  the same with the two keys of different kinds: ARP and ND (twice, once with each of them
        first in the batch), and an ARP request and an ARP reply of the same sender bytes
    G4  keys that start at slot `mask` (and one at slot 0): the chain crosses to slot 0; in a batch
        of n <= 64 (128 slots) and in one of 1,024 frames (2,048 slots)
    G5  is a sequence of calls (tests/test_gpu_learn_sets.py); its batches are G64 and G1024

Tiles, waves and lanes run in any order, so which of two colliding keys owns a slot is not known:
every condition has both keys in the batch, and the events must be right either way.  The expected
outputs of a batch come from learn_ref alone; the conditions are stated on set positions and
checked by tests/test_learn_sets.py on the keys learn_ref gives for the frames."""
import struct

import numpy as np

import learn_ref as L
import nd_ref as N
import respond_ref as R
from emurx import abi, frames as F

TILE, WAVE, LDS_SLOTS = 256, 64, 512
SEED = 0x5E75
NCAND = 1 << 19  # candidates per search: a 16-bit condition is met by some eight of them

_C = [np.uint64(c) for c in (0x9E3779B1, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F, 0x165667B1)]
_M32 = np.uint64(0xFFFFFFFF)


def hash_words(ns, ip0, ip1, ip2, ip3, mlo, mhk):
    """lrn_hash over the key's seven words; numpy uint64 arrays (values < 2^32) or scalars."""
    ns, ip0, ip1, ip2, ip3, mlo, mhk = (np.asarray(x, np.uint64) for x in (ns, ip0, ip1, ip2, ip3, mlo, mhk))
    s15, s13, s16 = np.uint64(15), np.uint64(13), np.uint64(16)
    h = ((ns * _C[0]) & _M32) ^ mhk
    h = ((h ^ ip0) * _C[1]) & _M32
    h = ((h ^ (h >> s15) ^ ip1) * _C[2]) & _M32
    h = ((h ^ (h >> s13) ^ ip2) * _C[3]) & _M32
    h = ((h ^ (h >> s16) ^ ip3) * _C[4]) & _M32
    h = ((h ^ (h >> s15) ^ mlo) * _C[1]) & _M32
    return h ^ (h >> s16)


def key_words(key):
    """learn_ref's key (ns, kind, 16 IP bytes, 6 MAC bytes) -> the seven words the kernels hold."""
    ns, kind, ip, mac = key
    return (ns,) + struct.unpack("<4I", ip) + (struct.unpack("<I", mac[:4])[0], struct.unpack("<H", mac[4:])[0] | kind << 16)


def key_hash(key) -> int:
    return int(hash_words(*key_words(key)))


def lds_start(h: int) -> int:
    return (h >> 9) & (LDS_SLOTS - 1)


def slots_of(n: int) -> int:
    """The global set's slot count for a batch of n frames (emurx_lrn_slots)."""
    s = 128
    while s < 2 * n and s < 1 << 27:
        s <<= 1
    return s


def tag(h: int) -> int:
    return h >> 27


# ---- the key families ---------------------------------------------------------------------------
ND_MAC = bytes([0, 0x10, 0x94, 0, 0, 9])
NS_PREFIX = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xEE]) + bytes(6)
NA_PREFIX = bytes([0x20, 1, 0x0D, 0xB8, 0, 0xEF]) + bytes(6)


def arp_key(ns, kind, j, m=None):
    m = j if m is None else m
    return (ns, kind, bytes([48, (j >> 16) & 255, (j >> 8) & 255, j & 255]) + bytes(12),
            bytes([0, 0x10, 0x94, (m >> 16) & 255, (m >> 8) & 255, m & 255]))


def nd_key(ns, kind, c, mac=ND_MAC):
    """ns: nd_ref's Namespace index (its id is N.NS_BASE + ns); c: the address' last four bytes."""
    return (N.NS_BASE + ns, kind, (NS_PREFIX if kind == abi.LRN_ND_NS else NA_PREFIX) + struct.pack(">I", c), mac)


def _be3(j):  # the three id bytes of j in a little-endian word's bytes 1..3 (byte 0 is the caller's)
    j = np.asarray(j, np.uint64)
    return ((j >> np.uint64(16)) & np.uint64(255)) << np.uint64(8) | ((j >> np.uint64(8)) & np.uint64(255)) << np.uint64(16) | \
        (j & np.uint64(255)) << np.uint64(24)


def arp_hashes(ns, kind, j, m=None):
    """key_hash(arp_key(ns, kind, j[i], m[i])) for arrays j, m."""
    j = np.asarray(j, np.uint64)
    m = j if m is None else np.asarray(m, np.uint64)
    ip0 = np.uint64(48) | _be3(j)
    mlo = np.uint64(0x00941000) | ((m >> np.uint64(16)) & np.uint64(255)) << np.uint64(24)
    mhk = ((m >> np.uint64(8)) & np.uint64(255)) | (m & np.uint64(255)) << np.uint64(8) | np.uint64(kind << 16)
    return hash_words(ns, ip0, 0, 0, 0, mlo, mhk)


def nd_hashes(ns, kind, c):
    """key_hash(nd_key(ns, kind, c[i])) for an array c (ns: nd_ref's Namespace index)."""
    w = key_words(nd_key(ns, kind, 0))
    c = np.asarray(c, np.uint64)
    ip3 = (c >> np.uint64(24)) | ((c >> np.uint64(16)) & np.uint64(255)) << np.uint64(8) | \
        ((c >> np.uint64(8)) & np.uint64(255)) << np.uint64(16) | (c & np.uint64(255)) << np.uint64(24)
    return hash_words(w[0], w[1], w[2], w[3], ip3, w[5], w[6])


# ---- frames ---------------------------------------------------------------------------------------
def frame_of(key):
    """-> (frame, vport) that learn_ref folds into `key`."""
    ns, kind, ip, mac = key
    if kind <= abi.LRN_ARP_REPLY:
        cmac, ip4, _ = R._client(ns, 0)
        req = kind == abi.LRN_ARP_REQ
        f = R._eth(L.BCAST if req else cmac, mac, R._NS[ns], 0x0806, F.arp(kind, mac, ip[:4], bytes(6) if req else cmac, ip4), 0)
        return f + bytes(max(60 - len(f), 0)), 1
    k = ns - N.NS_BASE
    if kind == abi.LRN_ND_NS:
        return N.ns_frame(N._NS[k], 0, N.eui_of(N._client(k, 0)[0]), src=ip, opts=N.slla(mac)), N.VPORT
    return N.ns_frame(N._NS[k], 0, ip, src=NS_PREFIX + bytes([0, 0, 0, 1]), dst=N.ALL_NODES, edst=bytes([0x33, 0x33, 0, 0, 0, 1]),
                      typ=136, body=bytes([0x60, 0, 0, 0]) + ip + b"\x02\x01" + mac), N.VPORT


def filler_frame():
    """An ARP frame of operation 3: a candidate that learns nothing."""
    cmac, ip4, _ = R._client(0, 0)
    f = R._eth(L.BCAST, ND_MAC, R._NS[0], 0x0806, F.arp(3, ND_MAC, bytes([48, 0, 0, 1]), bytes(6), ip4), 0)
    return f + bytes(max(60 - len(f), 0)), 1


# ---- the search -----------------------------------------------------------------------------------
class Picker:
    """Seeded candidates of each family with their hashes; every pick is a key no earlier pick took."""

    def __init__(self, seed=SEED):
        self.rng = np.random.default_rng(seed)
        self.used = set()
        self.fam = {}

    def family(self, name):
        """name: ("arp", ns, kind) or ("nd", ns, kind) -> (ids, hashes), ids seeded and distinct."""
        if name not in self.fam:
            what, ns, kind = name
            ids = self.ids(24 if what == "arp" else 32)
            h = arp_hashes(ns, kind, ids) if what == "arp" else nd_hashes(ns, kind, ids)
            self.fam[name] = (ids, h)
        return self.fam[name]

    def ids(self, bits):
        """NCAND seeded ids below 2^bits, distinct, in seeded order."""
        ids = np.unique(self.rng.integers(1, 1 << bits, NCAND, dtype=np.uint64))
        return ids[self.rng.permutation(len(ids))]

    def key(self, name, i):
        what, ns, kind = name
        return arp_key(ns, kind, int(i)) if what == "arp" else nd_key(ns, kind, int(i))

    def take(self, key):
        assert key not in self.used, key
        self.used.add(key)
        return key

    def one(self, name, sel):
        """The first unused key of the family whose hash meets sel (hashes -> bool array)."""
        ids, h = self.family(name)
        for i in np.nonzero(sel(h))[0]:
            k = self.key(name, ids[i])
            if k not in self.used:
                return self.take(k)
        raise AssertionError(("no candidate", name))

    def some(self, name, count):
        """The family's first `count` unused keys."""
        out = []
        for i in self.family(name)[0]:
            k = self.key(name, i)
            if k not in self.used:
                out.append(self.take(k))
                if len(out) == count:
                    return out
        raise AssertionError(("no candidates", name))

    def pair(self, a, b, sig):
        """Keys of families a and b (a may be b) with equal sig(hashes), both unused."""
        ia, ha = self.family(a)
        ib, hb = self.family(b)
        sa, sb = sig(ha), sig(hb)
        if a == b:
            order = np.argsort(sa, kind="stable")
            same = np.nonzero(sa[order][1:] == sa[order][:-1])[0]
            cand = [(order[x], order[x + 1]) for x in same]
        else:
            _, xa, xb = np.intersect1d(sa, sb, return_indices=True)
            cand = list(zip(xa, xb))
        for x, y in cand:
            ka, kb = self.key(a, ia[x]), self.key(b, ib[y])
            if ka not in self.used and kb not in self.used and ka != kb:
                return self.take(ka), self.take(kb)
        raise AssertionError(("no pair", a, b))


U = np.uint64
ARQ = lambda ns=0: ("arp", ns, abi.LRN_ARP_REQ)      # noqa: E731
ARP_ = lambda ns=0: ("arp", ns, abi.LRN_ARP_REPLY)   # noqa: E731
NNS = lambda ns=0: ("nd", ns, abi.LRN_ND_NS)         # noqa: E731
NNA = lambda ns=0: ("nd", ns, abi.LRN_ND_NA)         # noqa: E731


def _lds(h):
    return (h >> U(9)) & U(LDS_SLOTS - 1)


def _gsig(mask):  # the global set's start slot and tag in one word
    return lambda h: (h & U(mask)) | (h >> U(27)) << U(32)


def global_keys(pk: Picker, mask: int):
    """The placed keys of a global set of mask + 1 slots -> {condition: [keys]}."""
    out = {}
    a = pk.one(ARQ(), lambda h: (h & U(mask)) != U(mask))
    ha = key_hash(a)
    out["G1"] = [a, pk.one(ARQ(1), lambda h: ((h & U(mask)) == U(ha & mask)) & ((h >> U(27)) != U(tag(ha))))]
    out["G2-arp"] = list(pk.pair(ARQ(), ARQ(), _gsig(mask)))
    out["G2-nd"] = list(pk.pair(NNS(), NNS(), _gsig(mask)))
    # one IP, two MACs: the second MAC is searched for the first key's slot and tag
    b = pk.some(ARP_(2), 1)[0]
    j = int.from_bytes(b[2][1:4], "big")
    ms = pk.ids(24)
    hm = arp_hashes(2, abi.LRN_ARP_REPLY, np.full(len(ms), j, np.uint64), ms)
    hb = key_hash(b)
    m = next(int(x) for x in ms[_gsig(mask)(hm) == _gsig(mask)(np.asarray([hb], np.uint64))[0]] if int(x) != j)
    out["G2-mac"] = [b, pk.take(arp_key(2, abi.LRN_ARP_REPLY, j, m))]
    out["G3-arp-first"] = list(pk.pair(ARQ(3), NNA(1), _gsig(mask)))
    out["G3-nd-first"] = list(pk.pair(NNS(2), ARP_(1), _gsig(mask)))
    # a request and a reply of the same sender bytes
    ids, hq = pk.family(ARQ())
    hp = arp_hashes(0, abi.LRN_ARP_REPLY, ids)
    i = next(int(x) for x in ids[_gsig(mask)(hq) == _gsig(mask)(hp)] if arp_key(0, abi.LRN_ARP_REQ, int(x)) not in pk.used)
    out["G3-req-reply"] = [pk.take(arp_key(0, abi.LRN_ARP_REQ, i)), pk.take(arp_key(0, abi.LRN_ARP_REPLY, i))]
    last = lambda h: (h & U(mask)) == U(mask)  # noqa: E731
    out["G4"] = [pk.one(ARQ(), last), pk.one(NNS(1), last), pk.one(ARP_(), last), pk.one(NNA(), lambda h: (h & U(mask)) == U(0))]
    return out


def _frames(keys):
    fill = filler_frame()
    made = {}
    fr, vp = [], []
    for k in keys:
        if k is not None and k not in made:
            made[k] = frame_of(k)
        f, v = fill if k is None else made[k]
        fr.append(f)
        vp.append(v)
    return fr, vp


def _tile_pairs(waves, singles=0):
    """One tile: per wave a list of keys, each twice (k0 .. km, k0 .. km); the last wave's last
    `singles` keys once."""
    out = []
    for w, ks in enumerate(waves):
        s = singles if w == len(waves) - 1 else 0
        out += ks + ks[:len(ks) - s]
    return out


def scenario(seed=SEED):
    """-> {batch name: dict(keys=[key or None per frame], placed={condition: [keys]})}; frames come
    from batch_frames().  Every batch has 64 to 1,024 frames."""
    pk = Picker(seed)
    sc = {}
    # ---- the workgroup set: L1, L2, L3 in tile 0 of a batch of two tiles
    k0 = pk.some(ARQ(), 1)[0]
    l1a = list(pk.pair(ARQ(), ARQ(1), lambda h: _lds(h)))
    l1b = list(pk.pair(ARP_(), NNS(), lambda h: _lds(h)))
    l2 = [pk.one(ARQ(2), lambda h: _lds(h) == U(511)), pk.one(NNA(), lambda h: _lds(h) == U(511)),
          pk.one(ARQ(), lambda h: _lds(h) == U(0))]
    t0 = [l1a[0]] * 32 + [k0] * 32 + [l1a[1]] * 32 + [k0] * 32 + [l2[0]] * 32 + [k0] * 32 + [l2[1]] * 32 + [l2[2]] * 16 + [k0] * 16
    t1 = [l1b[0]] * 48 + [k0] * 16 + [l1b[1]] * 48 + [k0] * 16 + (l1a + l2 + [k0, k0, k0]) * 16
    sc["L123"] = dict(keys=t0 + t1, placed={"L1": l1a + l1b, "L2": l2, "L3": [k0]})
    # ---- the switch (L4) and the crowded folding tile (L5)
    fams = [ARQ(), ARP_(1), NNS(), NNA(2)]
    waves = [pk.some(fams[w], 33) for w in range(4)]
    tail = [k0] * 40
    full = [k0] * 192 + [l1a[0]] * 64
    a2 = pk.some(NNS(1), 1)[0]
    two_of = lambda size: [a2 if i in (10, 50) else None for i in range(size)]  # noqa: E731
    sc["L4-full-128-256"] = dict(keys=_tile_pairs([w[:32] for w in waves]) + tail, tile=0, want=(128, 256))
    sc["L4-full-129-256"] = dict(keys=_tile_pairs([w[:32] for w in waves[:3]] + [waves[3]], singles=2) + tail, tile=0,
                                 want=(129, 256))
    sc["L4-full-1-2"] = dict(keys=two_of(256) + tail, tile=0, want=(1, 2))
    sc["L4-ragged-127-254"] = dict(keys=full + _tile_pairs([w[:32] for w in waves[:3]] + [waves[3][:31]]), tile=1, want=(127, 254))
    sc["L4-ragged-128-254"] = dict(keys=full + _tile_pairs([w[:32] for w in waves[:3]] + [waves[3][:32]], singles=2), tile=1,
                                   want=(128, 254))
    sc["L4-ragged-1-2"] = dict(keys=full + [a2, a2], tile=1, want=(1, 2))
    for k in sc:
        sc[k].setdefault("placed", {})
    # ---- the global set at 128 slots (one wave) and at 2,048 slots (four tiles)
    g64 = global_keys(pk, 127)
    ks = [k for c in g64.values() for k in c]
    assert len(ks) <= 32
    sc["G64"] = dict(keys=(2 * (ks + ks[::-1]))[:64], placed=g64, mask=127)
    g1k = global_keys(pk, 2047)
    ks = [k for c in g1k.values() for k in c]
    pool = pk.some(ARQ(1), 150) + pk.some(NNA(1), 150)
    rng = np.random.default_rng([seed, 1024])
    keys = []
    for t in range(4):  # every placed key in every tile, at seeded lanes among seeded pool keys
        tile = ks + [pool[int(x)] for x in rng.integers(0, len(pool), TILE - len(ks))]
        keys += [tile[int(x)] for x in rng.permutation(TILE)]
    sc["G1024"] = dict(keys=keys, placed=g1k, mask=2047)
    return sc


def batch_frames(batch):
    """-> (frames, vports) of a scenario batch."""
    return _frames(batch["keys"])


def load_tables(target, env4=None, env6=None):
    """learn_ref's tables: respond_ref's Namespaces on vport 1, nd_ref's on vport 2."""
    N.load_combined(target, env4, env6)


# ---- the conditions, computed from per-frame keys ------------------------------------------------
def tile_shape(keys, t):
    """(leaders, learners, distinct keys) of tile t: leaders = the waves' distinct keys, summed."""
    tile = keys[t * TILE:(t + 1) * TILE]
    waves = [tile[w * WAVE:(w + 1) * WAVE] for w in range(TILE // WAVE)]
    leaders = sum(len({k for k in w if k is not None}) for w in waves)
    return leaders, sum(k is not None for k in tile), len({k for k in tile if k is not None})


def folds(keys, t):
    leaders, learners, _ = tile_shape(keys, t)
    return learners > 0 and 2 * leaders <= learners


def wave_leaders(keys, t):
    """Per wave of tile t the set of keys it leads."""
    tile = keys[t * TILE:(t + 1) * TILE]
    return [{k for k in tile[w * WAVE:(w + 1) * WAVE] if k is not None} for w in range(TILE // WAVE)]


def displaced(keys, slots, start):
    """Linear probing of the distinct keys into `slots` slots -> (keys not at their start slot, 1 if
    a probe stepped from the last slot to slot 0).  The set of taken slots, and so whether the
    step happens, does not depend on the order of insertion."""
    own, moved, wrapped = {}, 0, 0
    for k in dict.fromkeys(keys):
        p = s = start(key_hash(k))
        while p in own:
            wrapped |= p == slots - 1
            p = (p + 1) % slots
        own[p] = k
        moved += p != s
    return moved, wrapped
