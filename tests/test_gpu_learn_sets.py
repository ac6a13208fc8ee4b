"""emurx_learn_dev on the placed-key scenario of tests/learn_sets.py: chains, wraps, owners with an
equal tag and owners of another kind in the workgroup's set and in the global set, the fold switch
on both sides (tests/test_learn_sets.py asserts that the batches reach each of them).  Every batch
through emurx_classify_dev and emurx_learn_dev on one handle, checked with test_gpu_learn.check
against learn_ref.learn_batch: events, outcome and d_info bit-exact, nothing written around them."""
import pytest

import learn_ref as L
import learn_sets as S
import nd_ref as N
import respond_ref as R
from emurx import abi, frames as F
from test_gpu_learn import check, finish, learn
from test_gpu_respond import classify

pytestmark = pytest.mark.gpu

BATCHES = ["L123", "L4-full-128-256", "L4-full-129-256", "L4-full-1-2", "L4-ragged-127-254", "L4-ragged-128-254",
           "L4-ragged-1-2", "G64", "G1024"]


@pytest.fixture(scope="module")
def placed(gpu_ok, oracle_built):
    """One handle of max_frames 4,096 (its set has 8,192 slots: every batch probes a prefix of it),
    every batch classified on it, and each batch's reference."""
    from emurx.rx import RxPath
    rx = RxPath(0, max_ns=16, max_clients=64, max_frames=1 << 12)
    rx.register_all()
    env6 = N.Env()
    S.load_tables(rx, R.Env(), env6)
    sc = S.scenario()
    assert list(sc) == BATCHES
    for b in sc.values():
        buf, desc = F.pack_frames(*S.batch_frames(b))
        b["tb"], b["td"], b["trec"], rec = classify(rx, buf, desc)
        b["want"] = L.learn_batch(buf, desc, rec, abi.LRNK_ALL, env6)
        b["n"] = len(desc)
        assert L.events_array(L.fold(b["keys"])).tobytes() == b["want"][1].tobytes()  # the frames learn the keys placed
    yield dict(rx=rx, sc=sc)
    rx.close()


def run(p, name, sync=True):
    b = p["sc"][name]
    return learn(p["rx"], b["tb"], b["td"], b["trec"], b["n"], max(len(b["want"][1]), 1), sync=sync)


@pytest.mark.parametrize("name", BATCHES)
def test_learn_placed(placed, name):
    check(run(placed, name), placed["sc"][name]["want"])


def test_learn_placed_masks_back_to_back(placed):
    """G5: 128 slots, 2,048 slots, 128 slots again on one stream without synchronising, then the
    workgroup-set batch: the emit pass of each call left no slot behind in either prefix."""
    order = ["G64", "G1024", "G64", "L123", "G1024"]
    assert S.slots_of(placed["sc"]["G64"]["n"]) == 128 and S.slots_of(placed["sc"]["G1024"]["n"]) == 2048
    got = [run(placed, name, sync=False) for name in order]
    for name, g in zip(order, got):
        check(finish(g), placed["sc"][name]["want"])
