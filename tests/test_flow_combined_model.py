"""tests/flow_combined_model.py (the attack monitors, then FlowGetFlowFromHash with PortScan_Detect inside, then FlowAdd's
syncount_accum) pinned on the CPU: with all-zero monitor rules it is FlowPortScanModel, with the detector off it is
AttackFlowModel, and hand-derived known answers at exception_freq 3.  The known answers (KATS), the generated sequence
(generated()) and the frozen scenario are also what the GPU tests of ppe_flow_combine run."""
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import flow_portscan_model as fpm
import portscan_model as psm
import pyoracle
import test_flow_portscan_model as tm
from attack_flow_model import AttackFlowModel
from attack_model import AttackModel
from flow_combined_model import FlowCombinedModel
from pktbuild import tcp_packet, udp_packet
from ppe import abi
from ppe.abi import ST

GOLDEN = Path(__file__).resolve().parent / "golden" / "flow_combined_v1.npz"
DROP = abi.ACL_RULE_ACTION_DROP
A, B, S = tm.A, tm.B, tm.S
SYN, ACK = tm.SYN, tm.ACK
OK, NOMEM, DETECTED, HOLD = psm.OK, psm.NOMEM, psm.DETECTED, psm.HOLD
P24, NOSYN, ADROP, AFW, FNOMEM = tm.P24, tm.NOSYN, tm.ADROP, tm.AFW, tm.FNOMEM
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
TCPSYN = abi.F_TCP | abi.F_SYN
syn, prime, hot = tm.syn, tm.prime, tm.hot
ZERO = (0, 0, 0)


def land(src, dport=80):
    """A TCP SYN with sip == dip (DP_Land_Attack_Monitor, dp_attack.c:464-484)."""
    return tcp_packet(src, src, 40000, dport, flags=SYN)


def udp80(src=A):
    return udp_packet(src, S, 5000, 80)


# Every scenario: tm.kat_rules() (FW to ports 80 and 443 and from them, default DROP), exception_freq 3, the detector's
# hold 100 s at 1000 cycles per second, the monitors' hold 600 s.  A step: the detector's clock (cycles, seconds; the
# seconds are also cfg.now_seconds and the monitors' clock), `tick`: DP_Attack_Info_Update at that second before the
# batch, `ports`: the batch's port bytes (none: no port array), `want`: per packet (status, flow bits, PortScan_Detect's
# answer or None = not called), `accum`: {port: (udp_accum, syn_accum, syncount_accum)} after the batch (ports not
# named: all zero), `ps`: the detector's result counts after the batch.  tm.prime / tm.hot make a source held (their
# comment derives the record); their five UDP packets pass the UDP monitor, which counts them.
KATS = {
    # a. port 0 drops land packets.  A has a record with three port changes (prime: last_dport 12, exception 3, last_cycle
    # and cycle 10000): a packet to a fourth port would be its next change.  Its land SYN to port 13 at cycle 10500 is
    # dropped in DecodeTCP (decode-tcp.c:162-173) and never reaches FlowHandlePacket: no PortScan_Detect call, so the
    # record keeps port 12, exception 3 and its cycle stamp 10000, the result counts stay at four OK; the land monitor
    # returns before syn_accum (dp_attack.c:464-484 precedes :641)
    "a_land_syn_of_a_scanner": dict(pd={0: dict(drop_pack=1, land=1)}, steps=[
        dict(prime(A), accum={0: (4, 0, 0)}, records={(A, 12, 3, 0, 10000, 10000, 0)}),
        dict(clock=(10500, 500), frames=[land(A, 13)], want=[(LAND, "", None)], accum={0: (4, 0, 0)}, flows=0,
             records={(A, 12, 3, 0, 10000, 10000, 0)}, ps=dict(ok=4, nomem=0, detected=0, hold=0, drop=0),
             totals=dict(land_drop=1))]),
    # b. a SYN the detector drops: A is held (prime, hot: hold 601), its SYN to port 80 at ts 501 passes the monitors
    # (all-zero rules: counted in syn_accum, dp_attack.c:641), misses, passes syn_check, and PortScan_Detect says HOLD:
    # 24, FlowAdd is never reached: syncount_accum +0, no flow
    "b_syn_dropped_by_the_detector": dict(steps=[
        dict(prime(A), accum={0: (4, 0, 0)}), dict(hot(A), accum={0: (5, 0, 0)}),
        dict(clock=(11500, 501), frames=[syn(A, 40000)], want=[(P24, "", HOLD)], accum={0: (5, 1, 0)}, flows=0,
             ps=dict(ok=4, nomem=0, detected=1, hold=1, drop=2))]),
    # c. two SYNs of one 5-tuple that both pass: the first creates the flow (FlowAdd: +1), the second finds it
    # (flow.c:196-201: no FlowAdd, +0, never at the detector); the SYN monitor saw both
    "c_two_syns_one_tuple": dict(steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000)] * 2, want=[(AFW, "FN", OK), (AFW, "F", None)],
             accum={0: (0, 2, 1)}, flows=1, records={(A, 80, 0, 0, 10000, 10000, 0)})]),
    # d. the creator is dropped by the detector and a later SYN of the tuple creates: tm.KATS' g with the two SYNs on
    # ports 1 and 2.  ts 600 < hold 601: HOLD, 24; ts 601: the hold is over, 14500 - 11000 >= 2 rate: the last branch, OK,
    # port 80 is forwarded: FlowAdd: the +1 lands on port 2, the later packet's; the SYN monitor counted one on each
    "d_later_syn_creates": dict(steps=[
        dict(prime(A), accum={0: (4, 0, 0)}), dict(hot(A), accum={0: (5, 0, 0)}),
        dict(clock=(14500, 502), ts=[600, 601], ports=[1, 2], frames=[syn(A, 40000)] * 2,
             want=[(P24, "", HOLD), (AFW, "FN", OK)], accum={0: (5, 0, 0), 1: (0, 1, 0), 2: (0, 1, 1)}, flows=1,
             records={(A, 80, 1, 0, 14500, 14500, 0)})]),
    # e. UDP flood at speed 0 on port 0.  Second 500: A's UDP packet to port 80 is counted (udppps still 0: not dropped),
    # is the source's first create (OK) and creates the flow (64-byte frame: one packet, 64 bytes).  The tick at 501 makes
    # udppps 1 > 0.  Two more packets of the live flow at cycle 13000: the first arms the hold (dp_attack.c:618-627), the
    # second is held (:606): both 28 ahead of FlowFind: the flow keeps one packet and last-seen 500, the detector's record
    # its cycle stamp 10000 and the counts one OK
    "e_udp_flood_on_a_live_flow": dict(td={0: dict(drop_pack=1, flood_udp=1, udp_speed=0)}, steps=[
        dict(clock=(10000, 500), frames=[udp80()], want=[(AFW, "FN", OK)], accum={0: (1, 0, 0)}, flows=1),
        dict(clock=(13000, 501), tick=501, frames=[udp80()] * 2, want=[(UDPF, "", None)] * 2, accum={0: (2, 0, 0)},
             flows=1, records={(A, 80, 0, 0, 10000, 10000, 0)}, ps=dict(ok=1, nomem=0, detected=0, hold=0, drop=0),
             table=[(A, S, 5000, 80, 17, 1, 0, 64, 0, 500)], totals=dict(udpflood_drop=2))]),
    # f. flow-pool room 1: A's SYN creates; B's SYN passes the monitors, the detector (first create: OK, the record
    # stepped) and the ACL, and FlowAdd finds the pool empty (flow.c:124-129, ahead of :151-154): FLOW_NOMEM, +0
    "f_syn_creator_nomem": dict(flow_capacity=1, steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000), syn(B, 40000)], want=[(AFW, "FN", OK), (FNOMEM, "", OK)],
             accum={0: (0, 2, 1)}, flows=1,
             records={(A, 80, 0, 0, 10000, 10000, 0), (B, 80, 0, 0, 10000, 10000, 0)})]),
    # g. syn_count 1 on port 0.  Two SYNs of A create two flows: syncount_accum 2.  The tick makes syncount 2 > 1: every
    # SYN on the port is 27 in DecodeTCP (dp_attack.c:673), behind syn_accum's count: B's SYN (a source without a record)
    # and A's SYN to a new port never reach the detector: B gets no record, A's keeps port 80 and cycle 10000
    "g_syncount_after_a_tick": dict(td={0: dict(drop_pack=1, syn_count=1)}, steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000), syn(A, 40001)], want=[(AFW, "FN", OK)] * 2,
             accum={0: (0, 2, 2)}, flows=2),
        dict(clock=(10400, 501), tick=501, frames=[syn(B, 40000), syn(A, 40002, sp=443)], want=[(SYNC, "", None)] * 2,
             accum={0: (0, 2, 0)}, flows=2, records={(A, 80, 0, 0, 10000, 10000, 0)},
             ps=dict(ok=2, nomem=0, detected=0, hold=0, drop=0), totals=dict(syncount_drop=2))]),
    # h. a batch wholly monitor-dropped: three land SYNs of three sources: neither table changes
    "h_all_dropped": dict(pd={0: dict(drop_pack=1, land=1)}, steps=[
        dict(clock=(10000, 500), frames=[land(A), land(B), land(S)], want=[(LAND, "", None)] * 3, accum={}, flows=0,
             records=set(), ps=dict(ok=0, nomem=0, detected=0, hold=0, drop=0), totals=dict(land_drop=3))]),
    # i. no port array: everything on port 0.  Port 1 would drop land packets and every UDP packet after the tick; port 0
    # has no rule: the UDP packet and the land SYN to port 80 both create their flows, counted on port 0
    "i_no_port_array": dict(pd={1: dict(drop_pack=1, land=1)}, td={1: dict(drop_pack=1, flood_udp=1, udp_speed=0)}, steps=[
        dict(clock=(10000, 500), frames=[udp80()], want=[(AFW, "FN", OK)], accum={0: (1, 0, 0)}, flows=1),
        dict(clock=(10000, 501), tick=501, frames=[udp80(B), land(A)], want=[(AFW, "FN", OK)] * 2,
             accum={0: (1, 1, 1)}, flows=3)]),
}


def kat_model(k):
    o = pyoracle.Oracle(tm.kat_rules(), default_action=DROP)
    ps = psm.PortScanModel(able=1, action=0, exception_freq=3, hold_seconds=100, capacity=k.get("ps_capacity", 100),
                           cycles_per_second=tm.RATE)
    fp = fpm.FlowPortScanModel(o, k.get("flow_capacity", 100), ps)
    return o, FlowCombinedModel(o, AttackModel(k.get("pd"), k.get("td"), 600), fp)


def check_kat_state(step, accum, info, flows, records, ps_info, table, what):
    """The step's stated state against one side's (the model's, or the engine's)."""
    for p in range(4):
        assert accum[p] == step["accum"].get(p, ZERO), (what, "port", p)
    for key, v in step.get("totals", {}).items():
        assert info[key] == v, (what, key)
    if "flows" in step:
        assert flows == step["flows"], what
    if "records" in step:
        assert records == step["records"], what
    for key, v in step.get("ps", {}).items():
        assert ps_info[key] == v, (what, key)
    if "table" in step:
        assert table == step["table"], what


def accums(ai):
    return [(a["udp_accum"], a["syn_accum"], a["syncount_accum"]) for a in ai]


@pytest.mark.parametrize("name", sorted(KATS))
def test_known_answers(name):
    k = KATS[name]
    o, m = kat_model(k)
    for j, step in enumerate(k["steps"]):
        if "tick" in step:
            m.atk.tick(step["tick"])
        m.atk.clock(step["clock"][1])
        m.fp.ps.clock(*step["clock"])
        hdr, lens = tm.stack(step["frames"])
        ts = np.array(step["ts"], np.uint64) if "ts" in step else None
        ports = np.array(step["ports"], np.uint8) if "ports" in step else None
        got = m.classify_batch(hdr, lens, ports, ts, cfg=o.cfg(0, 1, step["clock"][1]))
        tm.check_step(step, got, (name, j))
        assert got["results"].tolist() == [-1 if r is None else r for _, _, r in step["want"]], (name, j)
        check_kat_state(step, accums(m.atk.ai), m.info(), len(m.fp.flows), m.fp.ps.records(), m.fp.ps.info(), m.table(),
                        (name, j))


# ---- the generated sequence ----
# fpm.gen_sequence's population and clock; on top of it a port byte per packet, some SYNs made land packets, a tick of
# the monitors wherever the second moves.  Port 0 drops land packets; port 1 is the UDP-flood port (a threshold the
# batches straddle); port 2 has the count monitor at 1 created flow per second; port 3 has no rule.
GEN_PD = {0: dict(drop_pack=1, land=1)}
GEN_TD = {1: dict(drop_pack=1, flood_udp=1, udp_speed=4, flood_syn=1, syn_speed=1 << 30, syn_count=1 << 30),
          2: dict(drop_pack=1, syn_count=1)}
GEN_HOLD = 1
GEN_FLOWS = 128      # (the flow pool: a few batches fill it, the aging empties it again)
SEED, BATCHES, MAX_N = 2057, 60, 130
NEEDED = ("a", "b", "c", "d", "e", "f", "g")
_cache = {}


def gen_combined(seed, batches, max_n):
    seq, par = fpm.gen_sequence(seed, batches, max_n, flow_capacity=GEN_FLOWS)
    rng = np.random.default_rng(seed + 1)
    last = None
    for s in seq:
        n = len(s["lens"])
        s["ports"] = rng.integers(0, 4, n).astype(np.uint8)
        hdr = s["hdr"]
        for i in np.flatnonzero(rng.random(n) < 0.08):   # (untagged IPv4, ihl 5: TCP flags at byte 47)
            if hdr[i, 23] == 6 and hdr[i, 47] & 0x02:
                hdr[i, 30:34] = hdr[i, 26:30]
                s["ports"][i] = 0 if rng.random() < 0.8 else s["ports"][i]
        # a SYN again a few packets later, on another port and two seconds on (the detector's hold is two seconds): both
        # pass, or the first is dropped by the detector and the second creates the flow
        for i in np.flatnonzero(rng.random(n) < 0.1):
            j = i + int(rng.integers(1, 9))
            if j < n and hdr[i, 23] == 6 and hdr[i, 47] == 0x02 and not (hdr[i, 30:34] == hdr[i, 26:30]).all():
                hdr[j], s["lens"][j] = hdr[i], s["lens"][i]
                s["ts"][j], s["ports"][j] = s["ts"][i] + 2, (s["ports"][i] + 1 + int(rng.integers(3))) & 3
        s["tick"] = last is not None and s["now_s"] != last
        last = s["now_s"]
    return seq, par


def generated():
    if "seq" not in _cache:
        _cache["seq"] = gen_combined(SEED, BATCHES, MAX_N)
    return _cache["seq"]


def gen_model(par, pd=GEN_PD, td=GEN_TD, able=1):
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)
    ps = psm.PortScanModel(able, 0, par["freq"], par["hold"], par["ps_capacity"], par["rate"])
    fp = fpm.FlowPortScanModel(o, par["flow_capacity"], ps)
    return o, FlowCombinedModel(o, AttackModel(pd, td, GEN_HOLD), fp)


def tally(ev, o, m_flows_before, records_before, s, out, cfg):
    """Counts the cases a-g of the known answers in one batch's result."""
    dec = o.classify_batch(s["hdr"], s["lens"], cfg=cfg)   # (stateless: the 5-tuples of the dropped packets too)
    st, fl = out["verdict"] & 0xFF, out["verdict"] >> 16
    keys, syn_creator, dropped_syn = [], {}, {}
    for i in range(len(st)):
        sip, dip, w2, w3 = (int(x) for x in dec["tuple"][i])
        key = fpm.flow_key(sip, dip, w2 & 0xFFFF, w2 >> 16, w3 & 0xFF)
        keys.append(key)
        port, is_syn = int(s["ports"][i]) & 3, (int(fl[i]) & TCPSYN) == TCPSYN
        if st[i] == LAND and sip in records_before:
            ev["a"] += 1
        if st[i] == P24 and is_syn:
            ev["b"] += 1
            dropped_syn.setdefault(key, port)
        if st[i] == AFW and is_syn and int(fl[i]) & abi.F_NEWFLOW:
            syn_creator[key] = i
            if key in dropped_syn and dropped_syn[key] != port:
                ev["d"] += 1
        elif st[i] == AFW and is_syn and key in syn_creator:
            ev["c"] += 1
        if st[i] == UDPF and key in m_flows_before:
            ev["e"] += 1
        if st[i] == FNOMEM and is_syn and out["results"][i] != -1:
            ev["f"] += 1
        if st[i] == SYNC:
            ev["g"] += 1


def run_generated(seq, par, pd=GEN_PD, td=GEN_TD, able=1, ev=None):
    """The model over the sequence: per batch its result; the model itself."""
    o, m = gen_model(par, pd, td, able)
    outs = []
    for s in seq:
        if s["tick"]:
            m.atk.tick(s["now_s"])
        m.atk.clock(s["now_s"])
        m.fp.ps.clock(s["now_c"], s["now_s"])
        cfg = o.cfg(0, 1, s["now_s"])
        before, recs = set(m.fp.flows), set(m.fp.ps.table)
        outs.append(m.classify_batch(s["hdr"], s["lens"], s["ports"], s["ts"], cfg))
        if ev is not None:
            tally(ev, o, before, recs, s, outs[-1], cfg)
        if s["age"]:
            m.age(s["now_s"], 2)
            m.fp.ps.timeout(s["now_c"])
    return outs, m


def test_generated_sequence_holds_every_case():
    """A condition on the inputs, from the model alone: each of the cases a-g occurs at least 10 times over the
    generated sequence, every monitor status occurs, the ticks and the aging act, and the flows aged out alone exceed a
    quarter of the 1,024 slots a table of this capacity and batch size has (so the engine's table must rehash)."""
    seq, par = generated()
    ev = Counter()
    outs, m = run_generated(seq, par, ev=ev)
    assert all(ev[k] >= 10 for k in NEEDED), dict(ev)
    st = np.concatenate([o["verdict"] & 0xFF for o in outs])
    assert {LAND, UDPF, SYNC, P24, FNOMEM, NOSYN, ADROP, AFW} <= set(st.tolist())
    assert sum(s["tick"] for s in seq) >= 10 and m.fp.del_flow > 256 and m.fp.ps.counts["del_pcb"] >= 1
    assert max(len(s["lens"]) for s in seq) == MAX_N and min(len(s["lens"]) for s in seq) == 1


def test_all_zero_rules_equal_the_detector_model():
    """No monitor rule: nothing is dropped ahead of the table, so rows, counters and both tables are
    FlowPortScanModel's over the same batches; the accumulators still count."""
    seq, par = generated()
    outs, m = run_generated(seq, par, pd=None, td=None)
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)
    ref = fpm.FlowPortScanModel(o, par["flow_capacity"],
                                psm.PortScanModel(1, 0, par["freq"], par["hold"], par["ps_capacity"], par["rate"]))
    for b, (s, got) in enumerate(zip(seq, outs)):
        ref.ps.clock(s["now_c"], s["now_s"])
        want = ref.classify_batch(s["hdr"], s["lens"], s["ts"], o.cfg(0, 1, s["now_s"]))
        for key in ("verdict", "flow_hash", "acl_hit", "tuple", "counters", "results"):
            assert np.array_equal(got[key], want[key]), (b, key)
        assert len(got["dropped"]) == 0
        if s["age"]:
            ref.age(s["now_s"], 2)
            ref.ps.timeout(s["now_c"])
    assert m.table() == ref.table() and m.stats() == ref.stats()
    assert m.fp.ps.records() == ref.ps.records() and m.fp.ps.info() == ref.ps.info()
    assert sum(a["udppps"] + a["synpps"] + a["syncount"] + a["udp_accum"] + a["syn_accum"] for a in m.atk.ai) > 0


def test_detector_off_equals_the_monitor_model():
    """able = 0: AttackFlowModel (the monitors ahead of pyoracle.OracleFlow) over the same batches: rows, counters, the
    flow table, the monitors' state."""
    seq, par = generated()
    outs, m = run_generated(seq, par, able=0)
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)
    ref = AttackFlowModel(o, par["flow_capacity"], AttackModel(GEN_PD, GEN_TD, GEN_HOLD))
    try:
        for b, (s, got) in enumerate(zip(seq, outs)):
            if s["tick"]:
                ref.atk.tick(s["now_s"])
            ref.atk.clock(s["now_s"])
            want = ref.classify_batch(s["hdr"], s["lens"], s["ports"], cfg=o.cfg(0, 1, s["now_s"]))
            for key in ("verdict", "flow_hash", "acl_hit", "tuple", "counters", "dropped"):
                assert np.array_equal(got[key], want[key]), (b, key)
            assert (got["results"] == -1).all()
            if s["age"]:
                ref.age(s["now_s"], 2)
        d = ref.ft.dump()
        cols = ("sip", "dip", "sport", "dport", "protocol", "pktcnts2d", "pktcntd2s", "bytecnts2d", "bytecntd2s",
                "last_seen")
        assert m.table() == sorted(tuple(int(x) for x in r) for r in zip(*(d[c] for c in cols)))
        assert m.stats() == ref.ft.stats() and m.info() == ref.info() and not m.fp.ps.table
        assert any(m.atk.totals.values())
    finally:
        ref.close()


# ---- the frozen scenario ----
def state_rows(m):
    """The monitors' state and totals as one array."""
    return np.array([[a[k] for k in abi.ATTACK_STATE_FIELDS] for a in m.atk.ai] +
                    [[m.atk.totals[k] for k in abi.ATTACK_TOTALS] + [0] * (len(abi.ATTACK_STATE_FIELDS) - 4)], np.uint64)


def test_frozen_scenario():
    """One generated scenario frozen as model output (tests/golden/flow_combined_v1.npz, written by
    tests/golden/gen_flow_combined_golden.py): the composition, the generator and the models under it have not moved."""
    g = np.load(GOLDEN)
    seq, par = gen_combined(int(g["seed"]), int(g["batches"]), int(g["max_n"]))
    outs, m = run_generated(seq, par)
    assert sum(len(s["lens"]) for s in seq) == len(g["verdict"]) and 200 <= len(g["verdict"]) <= 900
    for key in ("verdict", "flow_hash", "acl_hit", "results"):
        assert np.array_equal(np.concatenate([o[key] for o in outs]), g[key]), key
    assert np.array_equal(sum(o["counters"] for o in outs), g["counters"])
    assert np.array_equal(np.array(m.table(), np.uint64).reshape(-1, 10), g["flows"])
    assert np.array_equal(np.array(sorted(m.fp.ps.records()), np.uint64).reshape(-1, 7), g["records"])
    assert np.array_equal(state_rows(m), g["attack"])
