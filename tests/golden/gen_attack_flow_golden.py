"""Writes tests/golden/attack_flow_v1.npz: one scripted multi-batch scenario of tests/attack_flow_model.py (the attack
monitors ahead of the oracle's flow table) with ticks and aging between the batches, frozen, so that a change of the
model or of the oracle's flow table shows (tests/test_attack_flow.py replays it; tests/test_gpu_attack_flow.py runs it
on the GPU through ppe_flow_attack_attach).

Run from the repository root after the build: python tests/golden/gen_attack_flow_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle")]

import attack_model as am  # noqa: E402
from attack_flow_model import AttackFlowModel  # noqa: E402
from ppe import abi  # noqa: E402

HERE = Path(__file__).resolve().parent
NOW = 1_700_000_000
CAPACITY = 48          # small enough that the later batches run out of pool (FLOW_NOMEM)
TIMEOUT = 3            # aging: a flow idle for more than this many seconds goes
PD = {0: dict(drop_pack=1, land=1), 1: dict(drop_pack=1, land=2), 3: dict(drop_pack=0, land=1)}
TD = {0: dict(drop_pack=1, flood_udp=1, udp_speed=12, flood_syn=1, syn_speed=8, syn_count=1000),
      1: dict(drop_pack=1, flood_udp=2, udp_speed=0, flood_syn=0, syn_speed=0, syn_count=4),
      2: dict(drop_pack=2, flood_udp=1, udp_speed=0, flood_syn=1, syn_speed=0, syn_count=0),
      3: dict(drop_pack=1, flood_udp=1, udp_speed=15, flood_syn=1, syn_speed=3, syn_count=6)}
HOLD = 2
FLOW_DUMP = ("sip", "dip", "sport", "dport", "protocol", "pktcnts2d", "pktcntd2s", "bytecnts2d", "bytecntd2s", "last_seen")


def scenario():
    """("batch", now, kinds[], ports[], land[], host[]) / ("tick", now) / ("age", now): 7 seconds, two batches each;
    the packets draw their addresses from 24 hosts, so flows recur inside a batch and across batches."""
    rng = np.random.default_rng(20261021)
    steps = []
    for sec in range(7):
        for n in (37, 66):
            quiet = sec >= 5
            pool = np.array(("ack", "rst", "udp_lenerr", "syn_lenerr", "frag", "icmp") if quiet else
                            ("udp", "udp", "udp_short", "syn", "syn", "synack", "ack", "rst", "udp_lenerr", "frag"))
            m = 9 if quiet else n
            steps.append(("batch", NOW + sec, rng.choice(pool, m), rng.integers(0, 4, m).astype(np.uint8),
                          rng.random(m) < 0.15, rng.integers(0, 24, m)))
        steps.append(("tick", NOW + sec + 1))
        if sec in (3, 5):
            steps.append(("age", NOW + sec + 1))
    return steps


def frames_of(kinds, land, host):
    return [am.frame(k, 0x0A000001 + int(h), 0x0A000001 + int(h) if ld else 0x0B000001, vlan_tag=bool(i % 3 == 0),
                     dport=80 + int(h) % 3) for i, (k, ld, h) in enumerate(zip(kinds, land, host))]


def table(dump):
    rows = sorted(tuple(int(x) for x in r) for r in zip(*(dump[c] for c in FLOW_DUMP)))
    return np.array(rows, np.uint64).reshape(len(rows), len(FLOW_DUMP))


def run():
    import pyoracle
    o = pyoracle.Oracle(None, default_action=abi.ACL_RULE_ACTION_FW)
    m = AttackFlowModel(o, CAPACITY, am.AttackModel(PD, TD, HOLD))
    out = {}
    b = 0
    for step in scenario():
        if step[0] == "tick":
            m.atk.tick(step[1])
            continue
        if step[0] == "age":
            out[f"aged{b}"] = np.array([m.age(step[1], TIMEOUT)], np.uint64)   # (before batch b)
            continue
        _, now, kinds, ports, land, host = step
        m.atk.clock(now)
        hdr, lens = am.batch(frames_of(kinds, land, host))
        e = m.classify_batch(hdr, lens, ports, cfg=o.cfg(0, 1, now))
        info = m.info()
        out[f"kind{b}"] = np.array([am.KINDS.index(k) for k in kinds], np.uint8)
        out[f"port{b}"] = ports
        out[f"land{b}"] = land.astype(np.uint8)
        out[f"host{b}"] = host.astype(np.uint8)
        out[f"now{b}"] = np.array([now], np.uint64)
        for k in ("verdict", "flow_hash", "acl_hit", "counters"):
            out[f"{k}{b}"] = e[k]
        out[f"state{b}"] = np.array([[a[k] for k in abi.ATTACK_STATE_FIELDS] for a in info["ai"]], np.uint64)
        out[f"totals{b}"] = np.array([info[k] for k in abi.ATTACK_TOTALS], np.uint64)
        out[f"table{b}"] = table(m.ft.dump())
        b += 1
    out["nbatch"] = np.array([b], np.uint32)
    m.close()
    return out


if __name__ == "__main__":
    np.savez_compressed(HERE / "attack_flow_v1.npz", **run())
    print("wrote attack_flow_v1.npz")
