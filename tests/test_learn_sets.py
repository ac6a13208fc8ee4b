"""The placed-key scenario of tests/learn_sets.py on the host, no GPU: the restated hash against
emurx_learn_key_hash, the keys learn_ref folds the scenario's frames into against the keys the
frames were built for (records from the oracle), and every coverage condition, counted, on those
keys.  tests/test_gpu_learn_sets.py runs the same batches on the device: this test is what keeps
them from losing their power unnoticed."""
import ctypes as C

import numpy as np
import pytest

import learn_ref as L
import learn_sets as S
import nd_ref as N
from emurx import abi, frames as F


@pytest.fixture(scope="module")
def scen(oracle_built):
    """The scenario, and per batch the keys learn_ref gives its frames with the oracle's records."""
    import pyoracle
    o = pyoracle.Oracle()
    env6 = N.Env()
    S.load_tables(o, None, env6)
    sc = S.scenario()
    for b in sc.values():
        fr, vp = S.batch_frames(b)
        buf, desc = F.pack_frames(fr, vp)
        rec = o.rx_batch(buf, desc)[0]
        b["outcome"], b["ref_keys"] = L.learn_keys(buf, desc, rec, abi.LRNK_ALL, env6)
    return sc


def lib_hash(lib, key):
    return int(lib.emurx_learn_key_hash((C.c_uint32 * 7)(*S.key_words(key))))


def test_hash_restated(lib, scen):
    rng = np.random.default_rng(0x4A5)
    w = rng.integers(0, 1 << 32, (4000, 7), dtype=np.uint64)
    w[:1000, 2:5] = 0                # ARP keys: the IP's last three words are zero
    w[:, 6] &= 0x7FFFF               # the MAC's last two bytes | a kind of 1..4 << 16
    want = S.hash_words(*(w[:, k] for k in range(7)))
    for row, h in zip(w, want):
        assert lib.emurx_learn_key_hash((C.c_uint32 * 7)(*(int(x) for x in row))) == int(h)
    placed = {k for b in scen.values() for k in b["keys"] if k is not None}
    assert len(placed) > 400
    for k in placed:
        assert lib_hash(lib, k) == S.key_hash(k), k
    assert lib.emurx_learn_key_hash(None) == 0
    assert [S.slots_of(n) for n in (1, 64, 65, 1024, 1025, 4096)] == [128, 128, 256, 2048, 4096, 8192]


def test_frames_fold_into_their_keys(scen):
    for name, b in scen.items():
        assert 64 <= len(b["keys"]) <= 1024, name
        assert b["ref_keys"] == b["keys"], name
        assert all((o == abi.LRN_NONE) == (k is None) and (k is None or o == k[1]) for o, k in zip(b["outcome"], b["keys"])), name


def test_workgroup_set_conditions(scen):
    cov = {}
    b = scen["L123"]
    keys, p = b["ref_keys"], b["placed"]
    assert S.folds(keys, 0) and S.folds(keys, 1)
    lead = [S.wave_leaders(keys, t) for t in (0, 1)]
    n = 0
    for a, c in (p["L1"][0:2], p["L1"][2:4]):  # L1: equal start, different keys, led from different waves of one tile
        assert a != c and S.lds_start(S.key_hash(a)) == S.lds_start(S.key_hash(c))
        tiles = [t for t in (0, 1) if any(a in w and c not in w for w in lead[t]) and any(c in w and a not in w for w in lead[t])]
        assert tiles, (a, c)
        n += len(tiles)
    assert {a[1] for a in p["L1"]} >= {abi.LRN_ARP_REQ, abi.LRN_ARP_REPLY, abi.LRN_ND_NS}
    cov["L1"] = n
    s = [S.lds_start(S.key_hash(k)) for k in p["L2"]]  # L2: two leaders start at slot 511, one at slot 0
    assert s == [511, 511, 0] and len(set(p["L2"])) == 3
    assert all(any(k in w for w in lead[0]) for k in p["L2"])
    t0 = [k for k in dict.fromkeys(keys[:S.TILE])]
    assert S.displaced(t0, S.LDS_SLOTS, S.lds_start)[1] == 1  # whatever the order, a probe steps from slot 511 to slot 0
    cov["L2"] = 3
    k0 = p["L3"][0]  # L3: led by all four waves of a tile, and in a second tile
    assert all(k0 in w for w in lead[0]) and k0 in keys[S.TILE:]
    cov["L3"] = sum(k0 in w for t in (0, 1) for w in lead[t])
    cov["L4"] = {}
    for name, b in scen.items():  # L4: the switch, on both sides and at equality, full and ragged tiles
        if name.startswith("L4"):
            keys, t = b["ref_keys"], b["tile"]
            leaders, learners, distinct = S.tile_shape(keys, t)
            assert (leaders, learners) == b["want"], name
            assert S.folds(keys, t) == (b["want"] in ((128, 256), (127, 254), (1, 2))), name
            ragged = len(keys) % S.TILE != 0 and t == (len(keys) - 1) // S.TILE
            assert ragged == ("ragged" in name) and (ragged or len(keys) >= (t + 1) * S.TILE)
            assert len(keys) // S.TILE >= 1  # the other tile of the batch is there too
            cov["L4"][name[3:]] = (leaders, learners, int(S.folds(keys, t)))
    assert len(cov["L4"]) == 6 and sum(v[2] for v in cov["L4"].values()) == 4
    keys = scen["L4-full-128-256"]["ref_keys"]  # L5: a crowded folding tile
    leaders, learners, distinct = S.tile_shape(keys, 0)
    moved, _ = S.displaced([k for k in keys[:S.TILE]], S.LDS_SLOTS, S.lds_start)
    # 128 seeded keys in 512 slots: some 128 * 0.25 / 2 = 16 of them start in a taken slot (a
    # quarter of the slots fill up as the keys arrive); fewer than 8 would be another scenario
    assert S.folds(keys, 0) and distinct == 128 >= 100 and moved >= 8
    assert {k[1] for k in keys[:S.TILE]} == {1, 2, 3, 4}
    cov["L5"] = (distinct, moved)
    print("workgroup set coverage:", cov)


def test_global_set_conditions(scen):
    cov = {}
    for name in ("G64", "G1024"):
        b = scen[name]
        keys, p, mask = b["ref_keys"], b["placed"], b["mask"]
        assert S.slots_of(len(keys)) == mask + 1
        H = S.key_hash
        first = {k: keys.index(k) for k in dict.fromkeys(keys)}
        c = {}
        assert all(k in first for ks in p.values() for k in ks)
        a, d = p["G1"]
        assert a != d and H(a) & mask == H(d) & mask and S.tag(H(a)) != S.tag(H(d))
        c["G1"] = 1
        for cond, kinds in (("G2-arp", ({1, 2}, {1, 2})), ("G2-nd", ({3, 4}, {3, 4})), ("G2-mac", ({1, 2}, {1, 2})),
                            ("G3-arp-first", ({1, 2}, {3, 4})), ("G3-nd-first", ({3, 4}, {1, 2})),
                            ("G3-req-reply", ({abi.LRN_ARP_REQ}, {abi.LRN_ARP_REPLY}))):
            a, d = p[cond]
            assert a != d and H(a) & mask == H(d) & mask and S.tag(H(a)) == S.tag(H(d)), cond
            assert a[1] in kinds[0] and d[1] in kinds[1], cond
            if name == "G64":  # one wave: the pair's first key is at the lower lane
                assert first[a] < first[d], cond
            c[cond] = 1
        a, d = p["G2-arp"]
        assert a[1] == d[1]
        a, d = p["G2-nd"]
        assert a[1] == d[1]
        a, d = p["G2-mac"]
        assert (a[0], a[1], a[2]) == (d[0], d[1], d[2]) and a[3] != d[3]
        a, d = p["G3-req-reply"]
        assert (a[0], a[2], a[3]) == (d[0], d[2], d[3])
        s = [H(k) & mask for k in p["G4"]]
        assert s == [mask, mask, mask, 0] and len(set(p["G4"])) == 4
        assert S.displaced(keys, mask + 1, lambda h: h & mask)[1] == 1  # a probe steps from slot `mask` to slot 0
        c["G4"] = 3
        c["distinct"] = len(first)
        c["moved"] = S.displaced(keys, mask + 1, lambda h: h & mask)[0]
        cov[name] = c
    assert len(scen["G64"]["ref_keys"]) == 64 and len(scen["G1024"]["ref_keys"]) == 1024
    # G1024: every placed key in every tile, so that tiles meet each other's owners
    for t in range(4):
        tile = set(scen["G1024"]["ref_keys"][t * S.TILE:(t + 1) * S.TILE])
        assert all(k in tile for ks in scen["G1024"]["placed"].values() for k in ks)
    print("global set coverage:", cov)
