"""Extract the handler counters the reference's timestamp simulation recorded.

Source: /root/reference/unit-test/exp/icmp2.json, what TestPluginIcmp2 (src/emu/plugins/icmp/
icmp_test.go) dumped when it ended: six ICMPv4 timestamp requests, each answered.  The capture holds
no packets, because the replies carry the clock; this takes its "pktRx*" / "pktTx*" values, which
tests/test_ts_ref.py pins the timestamp rule of emurx_nsstat_ts_dev with.  Data only: names and
numbers.  Run where the reference is:

    python tests/golden/make_icmp2_counters.py

Writes tests/golden/icmp2_counters.json: {counter: value}.
"""
import json
from pathlib import Path

from make_nsstat_counters import walk

REF = Path("/root/reference/unit-test/exp/icmp2.json")
OUT = Path(__file__).resolve().parent / "icmp2_counters.json"


def main():
    out = {}
    walk(json.loads(REF.read_text()), out)
    OUT.write_text(json.dumps(dict(sorted(out.items())), indent=1, sort_keys=True) + "\n")
    print(out)


if __name__ == "__main__":
    main()
