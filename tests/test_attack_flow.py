"""The attack monitors on the flow-table path (ppe_flow_attack_attach) on the CPU: known answers of the tests' model
(tests/attack_flow_model.py = tests/attack_model.py's monitors ahead of pyoracle.OracleFlow) worked out by hand from
the reference lines the model cites, the frozen scenario, and the binding and the host-only planner entry through the
library.

The difference from the stateless path that these pin: DP_Attack_SynCountMonitor is called from FlowAdd behind
flow_item_alloc (flow.c:120-158), so syncount_accum counts the flows TCP SYN packets create, and a packet a monitor
drops (decode-ipv4.c:141-149, decode-tcp.c:162-173) never reaches FlowHandlePacket."""
import sys
from pathlib import Path

import numpy as np

import pyoracle
from attack_flow_model import AttackFlowModel
from attack_model import AttackModel, batch, frame
from pktbuild import eth, ipv4, tcp
from ppe import abi
from ppe.abi import ST

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
NOW = 1_700_000_000
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
FW, NOMEM, NOSYN, ADROP = ST["ACL_FW"], ST["FLOW_NOMEM"], ST["FLOW_TCP_NO_SYN_FIRST"], ST["ACL_DROP"]
A, B = 0x0A000001, 0x0B000002
NEW, FLOW, TOCL = abi.F_NEWFLOW, abi.F_FLOW, abi.F_TOCLIENT


def model(pd=None, td=None, capacity=16, hold=600, default_action=abi.ACL_RULE_ACTION_FW):
    o = pyoracle.Oracle(None, default_action=default_action)
    return AttackFlowModel(o, capacity, AttackModel(pd, td, hold))


def run(m, frames, ports=None, syn_check=1, now=NOW):
    """Statuses of one batch; the full result under run.last."""
    hdr, lens = batch(frames)
    run.last = e = m.classify_batch(hdr, lens, ports, cfg=m.o.cfg(0, syn_check, now))
    return (e["verdict"] & 0xFF).tolist()


def flags():
    return (run.last["verdict"] >> 16).tolist()


def accum(m, port=0):
    a = m.atk.ai[port]
    return a["udp_accum"], a["syn_accum"], a["syncount_accum"]


def dump(m):
    d = m.ft.dump()
    return sorted((int(r["sip"]), int(r["dip"]), int(r["sport"]), int(r["dport"]), int(r["pktcnts2d"]),
                   int(r["pktcntd2s"]), int(r["bytecnts2d"]), int(r["bytecntd2s"]), int(r["last_seen"])) for r in d)


def test_two_syns_of_one_tuple_count_one_creation():
    """1. The second SYN of the 5-tuple finds the flow the first created (flow.c:197-201): FlowAdd, and with it
    DP_Attack_SynCountMonitor, ran once.  Both passed DecodeTCP's SYN monitor: syn_accum 2.  The stateless model, where
    every packet is a flow miss, says 2: the difference is on record."""
    m = model()
    assert run(m, [frame("syn", A, B)] * 2) == [FW, FW]
    f = flags()
    assert f[0] & NEW and not f[1] & NEW and f[1] & FLOW
    assert accum(m) == (0, 2, 1)
    o, s = m.o, AttackModel()
    hdr, lens = batch([frame("syn", A, B)] * 2)
    s.expected(o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW)), hdr)
    assert (s.ai[0]["syn_accum"], s.ai[0]["syncount_accum"]) == (2, 2)
    m.close()


def test_syn_on_a_flow_of_an_earlier_batch():
    """2. syn_accum +1 (decode-tcp.c:162-173 runs for every SYN), syncount_accum +0 (FlowFind hit: no FlowAdd)."""
    m = model()
    assert run(m, [frame("syn", A, B)]) == [FW] and accum(m) == (0, 1, 1)
    assert run(m, [frame("syn", A, B)], now=NOW + 1) == [FW] and accum(m) == (0, 2, 1)
    assert flags()[0] & FLOW and not flags()[0] & NEW
    m.close()


def test_refused_creator_is_not_counted():
    """3. Capacity 1: the second new flow's flow_item_alloc fails (flow.c:124-129) before the monitor's call at :151."""
    m = model(capacity=1)
    assert run(m, [frame("syn", A, B), frame("syn", A + 1, B)]) == [FW, NOMEM]
    assert accum(m) == (0, 2, 1) and len(dump(m)) == 1
    m.close()


def test_only_tcp_syn_creations_count():
    """4. syn_check 0: an ACK-only packet creates its flow, and so does a UDP packet: FlowAdd's call is under
    TCP_IS_SYN (flow.c:151), neither counts; a SYN beside them does."""
    m = model()
    assert run(m, [frame("ack", A, B), frame("udp", A + 1, B), frame("syn", A + 2, B)], syn_check=0) == [FW, FW, FW]
    assert all(f & NEW for f in flags())
    assert accum(m) == (1, 1, 1) and len(dump(m)) == 3
    # with syn_check the ACK-only packet never reaches the ACL (flow.c:204-214): no flow, nothing counted
    m2 = model()
    assert run(m2, [frame("ack", A, B)]) == [NOSYN] and accum(m2) == (0, 0, 0) and dump(m2) == []
    m.close()
    m2.close()


def test_acl_dropped_syn_is_not_counted():
    """5. flow.c:232-243: the ACL's drop returns before FlowAdd: no flow, syn_accum 1, syncount_accum 0."""
    m = model(default_action=abi.ACL_RULE_ACTION_DROP)
    assert run(m, [frame("syn", A, B)]) == [ADROP]
    assert accum(m) == (0, 1, 0) and dump(m) == []
    m.close()


def test_monitor_drop_leaves_a_live_flow_untouched():
    """6. A SYN-flood drop and a land drop on live flows: DecodeTCP returns DECODE_DROP before FlowHandlePacket, so
    the flows' packet and byte counters and last-seen times stay; a non-SYN packet of the same flow in the same batch
    is found and counted."""
    m = model(td={0: dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)})
    syn, ack, land = frame("syn", A, B), frame("ack", A, B), frame("syn", A, A)
    assert run(m, [syn, land]) == [FW, FW]              # synpps 0: nothing drops yet; both flows created at NOW
    before = dump(m)
    assert [r[4] for r in before] == [1, 1] and [r[8] for r in before] == [NOW, NOW]
    m.atk.tick(NOW + 1)                                 # synpps 2 > syn_speed 0: the next interval's SYNs drop
    m.atk.set({0: dict(drop_pack=1, land=1)}, {0: dict(drop_pack=1, flood_syn=1, syn_speed=0, syn_count=1 << 30)})
    assert run(m, [syn, land], now=NOW + 5) == [SYNF, LAND]
    assert dump(m) == before
    assert flags() == [abi.F_TCP | abi.F_SYN] * 2       # no PPE_F_L4, no PPE_F_FLOW / TOCLIENT / NEWFLOW
    assert run.last["flow_hash"].tolist() == [0, 0] and run.last["acl_hit"].tolist() == [-1, -1]
    assert run.last["tuple"][:, 2].tolist() == [0, 0]
    cnt = dict(zip(abi.COUNTERS, run.last["counters"].tolist()))
    want = dict.fromkeys(abi.COUNTERS, 0)
    want.update(pkts=2, l2_rx_ok=2, ipv4_rx_ok=2, out_drop=2, rx_bytes=len(syn) + len(land))
    assert cnt == want
    assert m.atk.totals["synflood_drop"] == 1 and m.atk.totals["land_drop"] == 1
    assert run(m, [ack, syn], now=NOW + 6) == [FW, SYNF]
    after = dump(m)
    moved = [r for r in after if r not in before]
    assert len(moved) == 1 and moved[0][4] == 2 and moved[0][6] == len(syn) + len(ack) and moved[0][8] == NOW + 6
    m.close()


def test_land_dropped_syn_creates_no_flow():
    """7. The reverse-direction packet behind a land-dropped SYN is a miss: it creates the flow itself (PPE_F_NEWFLOW,
    no PPE_F_TOCLIENT), keyed in its own orientation.  (Non-SYN, syn_check 0: a SYN with sip == dip is land too.)"""
    def rev():
        l4 = tcp(80, 1234, 0x10, payload=b"\0" * 6)
        return eth(0x0800) + ipv4(6, A, A, len(l4)) + l4
    m = model(pd={0: dict(drop_pack=1, land=1)})
    assert run(m, [frame("syn", A, A), rev()], syn_check=0) == [LAND, FW]
    assert flags()[1] & NEW and not flags()[1] & TOCL
    d = dump(m)
    assert len(d) == 1 and d[0][:4] == (A, A, 80, 1234) and accum(m) == (0, 0, 0)
    # without the land rule the SYN creates the flow and the same packet finds it, towards the client
    m2 = model()
    assert run(m2, [frame("syn", A, A), rev()], syn_check=0) == [FW, FW]
    assert not flags()[1] & NEW and flags()[1] & TOCL and dump(m2)[0][:4] == (A, A, 1234, 80)
    m.close()
    m2.close()


def test_syncount_across_a_tick_is_the_created_flows():
    """8. Three flows created by SYNs, two more SYNs that find them, one refused creator (capacity 3): the tick moves 3
    into syncount (dp_attack.c:744-745).  syn_count 2 < 3: every SYN of the next interval is 27, those of live flows
    included, and their flows' counters stay."""
    m = model(td={0: dict(drop_pack=1, syn_count=2)}, capacity=3)
    fr = [frame("syn", A + i, B) for i in range(3)] + [frame("syn", A, B), frame("syn", A + 1, B), frame("syn", A + 9, B)]
    assert run(m, fr) == [FW] * 5 + [NOMEM]
    assert accum(m) == (0, 6, 3)
    m.atk.tick(NOW + 1)
    assert m.atk.ai[0]["syncount"] == 3 and m.atk.ai[0]["synpps"] == 6
    before = dump(m)
    assert run(m, [frame("syn", A, B), frame("syn", A + 20, B), frame("ack", A + 1, B)], now=NOW + 1) == [SYNC, SYNC, FW]
    assert m.atk.totals["syncount_drop"] == 2 and accum(m) == (0, 2, 0)
    assert [r for r in dump(m) if r[0] != A + 1] == [r for r in before if r[0] != A + 1]
    m.atk.tick(NOW + 2)                                # syncount 0 again: the count monitor lets go
    assert run(m, [frame("syn", A, B)], now=NOW + 2) == [FW]
    m.close()


def test_udp_flood_drops_a_live_udp_flow():
    """9. decode-ipv4.c:141-149: the UDP monitor sits before DecodeUDP and the flow table, so a flood drops the packets
    of a flow that exists, and the flow does not see them."""
    m = model(td={0: dict(drop_pack=1, flood_udp=1, udp_speed=0)})
    u = frame("udp", A, B)
    assert run(m, [u, u]) == [FW, FW]
    before = dump(m)
    assert len(before) == 1 and before[0][4] == 2
    m.atk.tick(NOW + 1)                                # udppps 2 > 0
    m.atk.clock(NOW + 1)
    assert run(m, [u, frame("udp_short", A, B)], now=NOW + 1) == [UDPF, UDPF]
    assert dump(m) == before and flags() == [0, 0]
    assert m.atk.ai[0]["udp_flood_hold"] == 1 and m.atk.ai[0]["udp_flood_hold_time"] == NOW + 601
    assert accum(m) == (2, 0, 0) and m.atk.totals["udpflood_drop"] == 2
    m.close()


def test_ports_keep_their_own_syncount():
    """The creation counts on the creating packet's input port (port & 3, as the engine takes it)."""
    m = model()
    fr = [frame("syn", A + i, B) for i in range(6)]
    assert run(m, fr, ports=np.array([0, 1, 2, 3, 5, 1], np.uint8)) == [FW] * 6
    assert [m.atk.ai[p]["syncount_accum"] for p in range(4)] == [1, 3, 1, 1]
    m.close()


def _gen():
    sys.path.insert(0, str(GOLDEN))
    try:
        import gen_attack_flow_golden as gen
    finally:
        sys.path.pop(0)
    return gen


def test_frozen_scenario():
    """The model reproduces tests/golden/attack_flow_v1.npz (gen_attack_flow_golden.py: ticks and aging between the
    batches), and the scenario reaches what it is there for."""
    gen = _gen()
    g = np.load(GOLDEN / "attack_flow_v1.npz")
    got = gen.run()
    assert sorted(got) == sorted(g.files)
    for k in g.files:
        assert got[k].dtype == g[k].dtype and np.array_equal(got[k], g[k]), k
    nb = int(g["nbatch"][0])
    v = np.concatenate([g[f"verdict{b}"] for b in range(nb)])
    st = v & 0xFF
    assert 300 <= len(v) <= 900
    assert all((st == s).sum() > 0 for s in (LAND, SYNF, SYNC, UDPF, NOMEM, NOSYN))
    assert ((v >> 16) & NEW).any() and ((v >> 16) & TOCL == 0).any() and ((v >> 16) & FLOW).any()
    assert sum(int(g[k][0]) for k in g.files if k.startswith("aged")) > 0
    # syncount_accum moved, and by less than the forwarded SYNs (the stateless count) somewhere
    need = abi.F_TCP | abi.F_SYN
    fw_syn = sum(int(((g[f"verdict{b}"] & 0xFF) == FW).__and__(((g[f"verdict{b}"] >> 16) & need) == need).sum())
                 for b in range(nb))
    created = sum(int((((g[f"verdict{b}"] >> 16) & (need | NEW)) == (need | NEW)).sum()) for b in range(nb))
    assert 0 < created < fw_syn


def test_binding_and_planner():
    """ppe_flow_attack_attach and ppe_pick_attack_flow are exported and bound; the planner entries over the four
    (flow, attached) pairs; a NULL context is refused without touching a device."""
    lib = abi.load()
    assert "ppe_flow_attack_attach" in abi.EXPORTS and "ppe_pick_attack_flow" in abi.EXPORTS
    assert hasattr(lib, "ppe_flow_attack_attach") and hasattr(lib, "ppe_pick_attack_flow")
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [lib.ppe_pick_attack_flow(f, a) for f, a in pairs] == [0, 0, 0, 1]
    assert [lib.ppe_pick_attack(f, a) for f, a in pairs] == [0, 1, 0, 0]
    assert lib.ppe_flow_attack_attach(None, None) == abi.PPE_EINVAL
    assert lib.ppe_abi_version() == 8
    hdr = (ROOT / "include" / "ppe_hip.h").read_text()
    assert "int  ppe_flow_attack_attach(ppe_ctx_t *ctx, ppe_attack_t *atk);" in hdr
