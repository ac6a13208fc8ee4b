"""The device's bucket walks on dense tables: the scenario of tests/dense_tables.py (spread 2;
chains of three and more buckets, the step from the last bucket to bucket 0, tombstones shipped as
delta blocks, removed and re-added keys; tests/test_dense_tables.py asserts that the batch reaches
each of them) through every caller of the walks, against the oracle and the Python references,
byte for byte.  Each test is one fresh child process (EMURX_TABLE_SPREAD is read once per process)
that runs one driver of dense_tables.py and prints one summary line."""
import pytest

from test_dense_tables import child

pytestmark = pytest.mark.gpu


def test_dense_classify(gpu_ok, oracle_built):
    """emurx_classify_dev at each staging size, emurx_rx_stream per 64-frame message and one ingest
    batch on each path: records, queues, counters and flow decisions equal the oracle's at n = 1,
    64, 65, 257 and the full batch, grouped and interleaved."""
    assert "classify runs=" in child("gpu_classify")


def test_dense_owner_lookup(gpu_ok, oracle_built):
    """emurx_parse_route_dev on one handle, emurx_lookup_dev on a second with the same tables: the
    owner-side probes (the hash carried in the head among them) give the oracle's records and flows."""
    assert "owner runs=" in child("gpu_owner_lookup")


def test_dense_respond(gpu_ok, oracle_built):
    """emurx_respond_kinds_dev: the ARP re-probe, the EUI-64 MAC probe with its RA-prefix check and
    the IPv6 probe through long chains, wraps and tombstones, against nd_ref / respond_ref; once
    more after a client left from the middle of each chain."""
    assert "respond runs=" in child("gpu_respond")


def test_dense_learn(gpu_ok, oracle_built):
    """emurx_learn_dev: the solicitation's source probe and the advertisement's target probe each
    see a hit and a miss through a chain, against learn_ref."""
    assert "learn runs=" in child("gpu_learn")
