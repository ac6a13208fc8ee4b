"""bench.py's rotating batch slots (permuted_batch): each slot is the workload's frames in a
seeded permutation at new addresses.  Checked on the CPU with torch CPU tensors and the
oracle: the slot's records are the original records in the permuted order (the parse depends
on a frame's bytes alone), every frame's bytes and ZMQ header moved intact, and the slots
occupy distinct bytes (no two slots share an address range)."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("cfg", ["B", "C", "E"])
def test_permuted_batch_is_the_same_workload(cfg, oracle_built):
    import torch
    from emurx import synth
    b = _bench()
    n = 3000
    w = {"B": lambda: synth.config_b(n), "C": lambda: synth.config_c(n), "E": lambda: synth.config_e(n)}[cfg]()
    buf = torch.from_numpy(w["buf"])
    o = oracle_built.Oracle()
    synth.load_tables(w, o)
    ref, _, _, _ = o.rx_batch(w["buf"], w["desc"])
    seed = 77
    pb, pd = b.permuted_batch(torch, buf, w["desc"], seed, "cpu")
    pbuf = pb.numpy()
    pdesc = pd.numpy().view(w["desc"].dtype)
    perm = np.random.default_rng(seed).permutation(n)
    # descriptors: same lengths / vports in permuted order, packed offsets (4-byte header gaps)
    assert np.array_equal(pdesc["len"], w["desc"]["len"][perm])
    assert np.array_equal(pdesc["vport"], w["desc"]["vport"][perm])
    seg = pdesc["len"].astype(np.int64) + 4
    assert pdesc["off"][0] == 4 and np.array_equal(np.diff(pdesc["off"].astype(np.int64)), seg[:-1])
    assert len(pbuf) == int(seg.sum()) + 64 and not pbuf[-64:].any()
    for k in (0, 1, n // 2, n - 1):  # frame bytes and their ZMQ headers moved intact
        so, po, ln = int(w["desc"]["off"][perm[k]]), int(pdesc["off"][k]), int(pdesc["len"][k])
        assert pbuf[po - 4:po + ln].tobytes() == w["buf"][so - 4:so + ln].tobytes()
    rec, _, _, _ = o.rx_batch(pbuf, pdesc)
    assert rec.tobytes() == ref[perm].tobytes()
    # another seed: another order
    pb2, _ = b.permuted_batch(torch, buf, w["desc"], seed + 1, "cpu")
    assert not torch.equal(pb2, pb)


def test_dump_outputs_writes_what_the_caller_reads(oracle_built, lib, tmp_path):
    """bench.py --dump-outputs on a step's outputs laid out as the device leaves them (32-byte
    records, per-tile queue segments with stale entries past each tile's count, tile counts, the
    sharded histogram after 3 batches): float arrays, the records' fields and the packed queues
    as the oracle gives them, one batch's share of the histogram; a seeded sample (the same in
    both dumps) once the batch is larger than the sample sizes."""
    import torch
    from emurx import abi, synth
    b = _bench()
    n = 3000
    w = synth.config_c(n)
    o = oracle_built.Oracle()
    synth.load_tables(w, o)
    orec, oq, oqoff, _ = o.rx_batch(w["buf"], w["desc"])
    nt, qcap = abi.ntiles(n), abi.queue_cap(n)
    ql = np.full((abi.NUM_QUEUES, qcap), 0x7EADBEEF, np.int32)
    tc = np.zeros((nt, 16), np.int32)
    for q in range(abi.NUM_QUEUES):
        for f in oq[oqoff[q]:oqoff[q + 1]].astype(np.int64):  # frame order within the queue
            t = f // abi.QUEUE_TILE
            ql[q, t * abi.QUEUE_TILE + tc[t, q]] = f
            tc[t, q] += 1
    per_batch = np.arange(2 * abi.HIST_BINS, dtype=np.int64) * 7
    hist = np.zeros((abi.HIST_SHARDS, 2 * abi.HIST_BINS), np.int64)
    hist[0], hist[-1] = per_batch, 2 * per_batch

    def snap():
        return dict(slot=1, batches=3, rec=torch.from_numpy(orec.view(np.uint8).copy()),
                    qlist=torch.from_numpy(ql.reshape(-1).copy()), tile_cnt=torch.from_numpy(tc.reshape(-1).copy()),
                    hist=torch.from_numpy(hist.reshape(-1).copy()))
    info = b.dump_outputs(tmp_path / "all", snap(), n, qcap, 0, 1)
    got = {f.stem: np.load(f) for f in (tmp_path / "all").glob("*.npy")}
    assert sorted(got) == info["arrays"] == ["histogram", "queue_offsets", "queues", "record_rows", "records"]
    assert all(v.dtype == np.float64 for v in got.values()) and info["bytes"] == sum(v.nbytes for v in got.values())
    want = np.stack([orec[k].astype(np.float64) for k in abi.REC_DTYPE.names], axis=1)
    assert np.array_equal(got["record_rows"], np.arange(n)) and np.array_equal(got["records"], want)
    assert np.array_equal(got["queues"], oq) and np.array_equal(got["queue_offsets"], oqoff)
    assert np.array_equal(got["histogram"], per_batch)
    # sampled: the same rows and positions in every dump, and the values at them
    for d in ("s1", "s2"):
        b.dump_outputs(tmp_path / d, snap(), n, qcap, 1, 2, sample=1000, queue_sample=1500)
    s1, s2 = ({f.stem: np.load(f) for f in (tmp_path / d).glob("*_rank1.npy")} for d in ("s1", "s2"))
    assert len(s1) == 6 and all(np.array_equal(s1[k], s2[k]) for k in s1)
    rows, pos = s1["record_rows_rank1"].astype(np.int64), s1["queue_rows_rank1"].astype(np.int64)
    assert len(np.unique(rows)) == 1000 and len(np.unique(pos)) == 1500
    assert np.array_equal(s1["records_rank1"], want[rows]) and np.array_equal(s1["queues_rank1"], oq[pos])
