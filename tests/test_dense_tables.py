"""The dense-table scenario (tests/dense_tables.py) on a host-only handle, no GPU: its bucket
counts, its coverage conditions (long chains, the step across the table's end, tombstones, removed
and re-added keys, in every table the device walks), emurx_image_probe against emurx_image_lookup
and against the builder's own dicts, and the oracle's records against what each frame was built
for.  tests/test_gpu_dense_tables.py runs the same scenario on the device: this test is what keeps
those from losing their power unnoticed.  One child process, because EMURX_TABLE_SPREAD is read
once per process."""
import ast
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PRELUDE = "import sys; sys.path[:0] = ['tests', 'trex-emu_amd', 'oracle']; import dense_tables as D; "


def child(call, timeout=300):
    import dense_tables as D
    out = subprocess.run([sys.executable, "-c", PRELUDE + f"print(D.{call}())"], cwd=ROOT, capture_output=True, text=True,
                         timeout=timeout, env={**os.environ, **D.ENV})
    assert out.returncode == 0, out.stderr[-4000:]
    line = out.stdout.strip().splitlines()[-1]
    assert line.startswith("ok "), out.stdout[-2000:]
    return line


def test_dense_scenario_on_host(lib, oracle_built):
    import dense_tables as D
    line = child("check_host")
    cov = ast.literal_eval(line.split("coverage=")[1])  # frames per condition, as the child counted them
    assert set(cov) == {D.TNAME[t] for t in D.WALKED} | {"ci"}
    for t in D.WALKED:
        assert all(cov[D.TNAME[t]][c] >= 1 for c in D.CONDITIONS), (D.TNAME[t], cov[D.TNAME[t]])
    assert cov["ci"]["first2"] >= 1 and cov["ci"]["eui_prefix2"] >= 1
