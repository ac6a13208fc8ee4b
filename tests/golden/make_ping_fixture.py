"""Extract what the reference's two ping simulations recorded.

Sources: /root/reference/unit-test/exp/icmp3.json (TestPluginIcmp3, src/emu/plugins/icmp/
icmp_test.go: icmp_c_start_ping, five echo requests, each answered) and ipv6ping_rpc.json (the
ipv6_start_ping simulation of src/emu/plugins/ipv6/ipv6_test.go).  This takes, per capture, the
five rx frames (the echo replies), the tunnel and the client of the RPC that started the ping, the
recorded icmp_ping_stats and the handler counters ("pktRx*" / "pktTx*").  Data only: frames as
hex, names and numbers.  Run where the reference is:

    python tests/golden/make_ping_fixture.py

Writes tests/golden/ping_fixture.json: {capture: {family, env, tun, mac, dst, rx, stats, counters}}.
"""
import json
from pathlib import Path

REF = Path("/root/reference/unit-test/exp")
OUT = Path(__file__).resolve().parent / "ping_fixture.json"
# capture -> (family, the environment of tests/sim_envs.py that its Go test builds)
CAPTURES = {"icmp3.json": (4, "icmp"), "ipv6ping_rpc.json": (6, "ipv6")}


def extract(name, family, env):
    out = dict(family=family, env=env, rx=[], counters={})
    for e in json.loads((REF / name).read_text()):
        if e.get("meta") == "rx":
            out["rx"].append(e["data"].replace("|", ""))
        elif "rpc-req" in e and e["rpc-req"]["method"].endswith("start_ping"):
            p = e["rpc-req"]["params"]
            out.update(tun=p["tun"], mac=p["mac"], dst=p["dst"], amount=p["amount"])
        elif "rpc-res" in e and isinstance(e["rpc-res"].get("result"), dict):
            out["stats"] = e["rpc-res"]["result"]["icmp_ping_stats"]
        elif "meta" not in e and "rpc-req" not in e and "rpc-res" not in e:
            out["counters"].update({k: v for k, v in e.items() if k.startswith(("pktRx", "pktTx"))})
    assert len(out["rx"]) == 5 and "stats" in out and "tun" in out, name
    return out


def main():
    fx = {name: extract(name, fam, env) for name, (fam, env) in CAPTURES.items()}
    OUT.write_text(json.dumps(fx, indent=1, sort_keys=True) + "\n")
    print({k: (v["stats"], v["counters"]) for k, v in fx.items()})


if __name__ == "__main__":
    main()
