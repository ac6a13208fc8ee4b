"""The tx planner's rule (tests/txplan_ref.py, include/emu_rx.h emurx_tx_plan_dev) against the
golden captures and against hand-built frames; no GPU.

The captures hold what the reference's send paths wrote: the plan of a captured frame, run
through the checksum reference on the frame with the planned fields cleared, must give the
captured bytes back, and must be the descriptor the capture's producer ran (tx_util)."""
import numpy as np
import pytest

import tx_ref
import tx_util
import txplan_cases
import txplan_ref
from emurx import abi
from test_oracle_corpus import corpus_batch


@pytest.fixture(scope="module")
def corpus():
    buf, desc, _ = corpus_batch()
    return buf, desc


def test_constants_and_struct_against_header():
    import ctypes as C
    import re
    txt = (abi.REPO_ROOT / "include" / "emu_rx.h").read_text()
    for name, val in (("TXP_UDP0_KEEP", abi.TXP_UDP0_KEEP), ("TXP_INFO_WORDS", abi.TXP_INFO_WORDS),
                      ("EGRESS_SLOTS", abi.EGRESS_SLOTS)):
        m = re.search(r"#define EMURX_%s (\d+)u?\b" % name, txt)
        assert m and int(m.group(1)) == val, name
    m = re.search(r"enum emurx_txp \{(.*?)\}", txt, re.S)
    got = {k: int(v) for k, v in re.findall(r"EMURX_TXP_(\w+) = (\d+)", m.group(1))}
    assert got == {"NONE": abi.TXP_NONE, "HDR": abi.TXP_HDR, "L4": abi.TXP_L4, "LENGTH": abi.TXP_LENGTH, "BAD": abi.TXP_BAD}
    assert C.sizeof(abi.EgressResult) == 48 + 8 * abi.TXP_INFO_WORDS == 112


def test_plans_are_the_capture_producers_descriptors(oracle_built):
    """With UDP0_KEEP the rule gives exactly the (l3, l4, osize, ops, nh) of every descriptor that
    tx_util derives from the parser's records of the captures."""
    buf, d, _, _ = tx_util.corpus_tx_cases()
    assert len(d) > 7000
    for x in d:
        p = buf[int(x["off"]):int(x["off"]) + int(x["len"])].tobytes()
        got = txplan_ref.plan_frame(p, abi.TXP_UDP0_KEEP)
        assert got[:5] == (int(x["l3"]), int(x["l4"]), int(x["osize"]), int(x["ops"]), int(x["nh"])), (got, x)
        assert got[5] in (abi.TXP_HDR, abi.TXP_L4, abi.TXP_LENGTH)


@pytest.mark.parametrize("flags", [0, abi.TXP_UDP0_KEEP])
def test_round_trip_over_every_capture_frame(corpus, flags):
    """Clear the fields the planned ops name, run the checksum reference, get the captured bytes
    back: every frame of the corpus.  (Without the flag a captured UDP frame whose field is zero
    is the exception the flag exists for, so that run leaves those frames out.)"""
    buf, desc = corpus
    txd, oc, info = txplan_ref.plan(buf, desc, flags)
    assert len(desc) > 8000 and int(info.sum()) == len(desc) and not info[abi.TXP_BAD]
    for o in (abi.TXP_NONE, abi.TXP_HDR, abi.TXP_L4, abi.TXP_LENGTH):
        assert info[o] == int((oc == o).sum()) > 0, o
    assert int((txd["ops"] != 0).sum()) == int(info[abi.TXP_HDR] + info[abi.TXP_L4] + (oc[txd["ops"] != 0] == abi.TXP_LENGTH).sum())
    out, st = tx_ref.tx_checksum(txplan_ref.clear_fields(buf, txd), txd)
    assert not st.any()
    keep_txd = txd if flags else txplan_ref.plan(buf, desc, abi.TXP_UDP0_KEEP)[0]
    for i, (x, k) in enumerate(zip(txd, keep_txd)):
        a, b = int(x["off"]), int(x["off"]) + int(x["len"])
        if not flags and x["ops"] != k["ops"]:  # a zero UDP field that this run computed
            f = a + int(x["l4"]) + 6
            assert bytes(buf[f:f + 2]) == b"\0\0" and bytes(out[f:f + 2]) != b"\0\0", i
            continue
        assert out[a:b].tobytes() == buf[a:b].tobytes(), i


CASES = txplan_cases.cases()


@pytest.mark.parametrize("name,frame,want,want_keep", CASES, ids=[c[0] for c in CASES])
def test_hand_built_frames(name, frame, want, want_keep):
    assert txplan_ref.plan_frame(frame, 0) == want
    assert txplan_ref.plan_frame(frame, abi.TXP_UDP0_KEEP) == want_keep
    # a planned frame is one the checksum call accepts, and what it writes the rx parser's sums accept
    for w in (want, want_keep):
        p = bytearray(frame)
        assert tx_ref.tx_frame(p, *w[:5]) == abi.TX_OK
        if w[5] in (abi.TXP_NONE, abi.TXP_BAD) or (w[5] == abi.TXP_LENGTH and not w[3]):
            assert w[:5] == (0, 0, 0, 0, 0) and p == frame


def test_hand_built_frames_cover_every_outcome_and_kind():
    seen = {w[5] for c in CASES for w in c[2:]}
    assert seen == {abi.TXP_NONE, abi.TXP_HDR, abi.TXP_L4, abi.TXP_LENGTH, abi.TXP_BAD}
    kinds = {w[3] >> abi.TX_L4_SHIFT for c in CASES for w in c[2:]}
    assert kinds == set(range(7))
    assert any(c[2] != c[3] for c in CASES)


def test_batch_form_counts_and_copies_off_len():
    for flags in (0, abi.TXP_UDP0_KEEP):
        buf, desc, want, oc = txplan_cases.batch(flags)
        txd, got_oc, info = txplan_ref.plan(buf, desc, flags)
        assert txd.tobytes() == want.tobytes() and np.array_equal(got_oc, oc)
        assert np.array_equal(info[:5], np.bincount(oc, minlength=5)) and not info[5:].any()
