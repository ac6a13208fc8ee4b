"""Extract the handler counters the reference's simulation captures recorded.

Source: /root/reference/unit-test/exp/<capture>.json: next to its frames a capture holds the
counter objects its Go test dumped when it ended (the plugins' stats, non-zero values only).  This
takes every "pktRx*" / "pktTx*" value of the captures tests/test_nsstat_ref.py pins
emurx_nsstat_dev's counters with.  Data only: names and numbers.  Run where the reference is:

    python tests/golden/make_nsstat_counters.py

Writes tests/golden/nsstat_counters.json: {capture: {counter: value}}; a capture that recorded no
such counter (ipv6nd_2, ipv6nd_3) maps to {}.
"""
import json
from pathlib import Path

REF = Path("/root/reference/unit-test/exp")
OUT = Path(__file__).resolve().parent / "nsstat_counters.json"
CAPTURES = ["arp2.json", "arp4.json", "arp5.json", "icmp1.json", "icmpv6_1.json", "icmpv6_2.json", "ipv6nd_2.json",
            "ipv6nd_3.json"]


def walk(x, out):
    if isinstance(x, dict):
        for k, v in x.items():
            if isinstance(v, int) and not isinstance(v, bool) and (k.startswith("pktRx") or k.startswith("pktTx")):
                assert out.setdefault(k, v) == v, k
            else:
                walk(v, out)
    elif isinstance(x, list):
        for v in x:
            walk(v, out)


def main():
    res = {}
    for name in CAPTURES:
        out = {}
        walk(json.loads((REF / name).read_text()), out)
        res[name] = dict(sorted(out.items()))
    OUT.write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(res)


if __name__ == "__main__":
    main()
