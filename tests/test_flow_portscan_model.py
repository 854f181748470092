"""tests/flow_portscan_model.py (FlowGetFlowFromHash with PortScan_Detect inside, flow.c:181-245) pinned three ways,
all on the CPU: against pyoracle.OracleFlow with the detector off, against PortScanModel.expected over the stateless
oracle when no flow can ever be created, and by hand-derived known answers.  The known answers (KATS) and the generated
sequence (generated()) are also what the GPU tests of ppe_flow_portscan_attach run."""
from pathlib import Path

import numpy as np
import pytest

import flow_portscan_model as fpm
import portscan_model as psm
import pyoracle
from pktbuild import tcp_packet, udp_packet
from ppe import abi
from ppe.abi import ST

GOLDEN = Path(__file__).resolve().parent / "golden" / "flow_portscan_v1.npz"
FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP
A, B, S = 0x0A000001, 0x0A000002, 0x0B000001
SYN, SYNACK, ACK = 0x02, 0x12, 0x10
RATE = 1000
OK, NOMEM, DETECTED, HOLD = psm.OK, psm.NOMEM, psm.DETECTED, psm.HOLD
P24, NOSYN, ADROP, AFW, FNOMEM = (ST["PORTSCAN_DROP"], ST["FLOW_TCP_NO_SYN_FIRST"], ST["ACL_DROP"], ST["ACL_FW"],
                                  ST["FLOW_NOMEM"])
BITS = {"": 0, "F": abi.F_FLOW, "FT": abi.F_FLOW | abi.F_TOCLIENT, "FN": abi.F_FLOW | abi.F_NEWFLOW}


def stack(frames, stride=64):
    hdr = np.zeros((len(frames), stride), np.uint8)
    for i, f in enumerate(frames):
        hdr[i, :len(f)] = np.frombuffer(f, np.uint8)
    return hdr, np.array([len(f) for f in frames], np.uint32)


def kat_rules():
    """FW to ports 80 and 443 and from them (the replies); the default is DROP."""
    r = np.zeros(4, abi.RULE_DTYPE)
    for k, p in enumerate((80, 443)):
        r[k]["sport_end"] = 65535
        r[k]["dport_start"] = r[k]["dport_end"] = p
        r[k + 2]["dport_end"] = 65535
        r[k + 2]["sport_start"] = r[k + 2]["sport_end"] = p
    r["protocol_end"] = 255
    r["action"] = FW
    return r


def syn(c, cp, fl=SYN, s=S, sp=80):
    return tcp_packet(c, s, cp, sp, flags=fl)


def reply(c, cp, fl=SYNACK, s=S, sp=80):
    return tcp_packet(s, c, sp, cp, flags=fl)


# A source is made "held" in two steps (exception_freq 3, hold 100 s, rate 1000 cycles):
#   prime  at cycle 10000, second 500: four UDP packets to ports 9-12, no rule: each a miss whose ACL verdict is DROP, so
#          no flow; the detector runs first (flow.c:215 precedes :232): first create (dp_portscan.c:155-160), then three
#          port changes in the `< rate` branch (:163-176, last_exception 0 < 3): OK x 4, exception 3, last_dport 12
#   hot    at cycle 11500, second 501: a UDP packet to port 13: 1500 lies between rate and 2 rate (:177-194):
#          last_cycle 11000, last_exception 3, exception 0; the port changed: exception 1 and, last_exception 3 >= 3,
#          hold = 501 + 100 = 601, DETECTED; action 0: status 24 (flow.c:216-230)
def prime(src):
    return dict(clock=(10000, 500), frames=[udp_packet(src, S, 5000, p) for p in (9, 10, 11, 12)],
                want=[(ADROP, "", OK)] * 4)


def hot(src, action=0):
    return dict(clock=(11500, 501), frames=[udp_packet(src, S, 5000, 13)],
                want=[(P24 if action == 0 else ADROP, "", DETECTED)])


KATS = {
    # a. a held source sends the same new 5-tuple twice: ts 501 < hold 601, HOLD (dp_portscan.c:143-148) both times: 24,
    # no ACL, no flow; the tuple's claimed slot is left reclaimable (no flow in the table).  Then cycle 14500 and ts 601:
    # the hold is over (:151); 14500 - 11000 >= 2 rate: the last branch (:195-206) zeroes both counts, the port changed:
    # exception 1, OK; the ACL forwards port 80: the flow is created
    "a_held_twice": dict(steps=[
        prime(A), hot(A),
        dict(clock=(11500, 501), frames=[syn(A, 40000)] * 2, want=[(P24, "", HOLD)] * 2, flows=0),
        dict(clock=(14500, 700), ts=[601], frames=[syn(A, 40000)], want=[(AFW, "FN", OK)], flows=1,
             records={(A, 80, 1, 0, 14500, 14500, 0)})]),
    # b. the window rolls at the batch's first packet.  Batch 1: the SYN is the source's first create (OK) and creates
    # flow 40000 -> 80; three UDP packets to ports 9-11 change the port three times.  Batch 2 at cycle 11500: a SYN of a new
    # tuple rolls the window (:177-194), last_exception 3 >= 3 and 80 != 11: DETECTED, hold 601; the same tuple again:
    # HOLD; the ACK of the flow created earlier is found (flow.c:196-201), never at the detector although its source
    # is held, and so is the server's reply (PKT_TO_CLIENT, :248-269)
    "b_window_rolls": dict(steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000)] + [udp_packet(A, S, 5000, p) for p in (9, 10, 11)],
             want=[(AFW, "FN", OK)] + [(ADROP, "", OK)] * 3),
        dict(clock=(11500, 501), frames=[syn(A, 40001), syn(A, 40001), syn(A, 40000, ACK), reply(A, 40000)],
             want=[(P24, "", DETECTED), (P24, "", HOLD), (AFW, "F", None), (AFW, "FT", None)], flows=1,
             records={(A, 80, 1, 3, 11000, 11500, 601)})]),
    # c. creator shift: the held client's SYN is dropped (HOLD); the server's SYN|ACK of the same tuple is then a miss; it
    # has SYN set, so syn_check lets it pass (:204-214); the detector judges it under the server's own record (first
    # create, OK); the ACL forwards source port 80: the flow is created oriented as the reply (sip S, sport 80, packet to
    # server by :252-255).  The client's ACK is found: its sport 40000 is not the flow's 80: PKT_TO_CLIENT
    "c_creator_shift": dict(steps=[
        prime(A), hot(A),
        dict(clock=(11500, 501), frames=[syn(A, 40000), reply(A, 40000), syn(A, 40000, ACK)],
             want=[(P24, "", HOLD), (AFW, "FN", OK), (AFW, "FT", None)], flows=1,
             records={(A, 13, 1, 3, 11000, 11500, 601), (S, 40000, 0, 0, 11500, 11500, 0)})]),
    # d. cross-source dependency, the other endpoint free: A's SYN creates the flow; the server's UDP packet to port 9 is its
    # first create; its SYN|ACK finds A's flow and never reaches the detector: the server's record keeps port 9,
    # exception 0
    "d_other_free": dict(steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000), udp_packet(S, B, 7, 9), reply(A, 40000)],
             want=[(AFW, "FN", OK), (ADROP, "", OK), (AFW, "FT", None)], flows=1,
             records={(A, 80, 0, 0, 10000, 10000, 0), (S, 9, 0, 0, 10000, 10000, 0)})]),
    # d'. the same three packets with A held: A's SYN is dropped, so the SYN|ACK is a miss and reaches the detector under
    # the server's record: port 40000 != 9 in the `< rate` branch: exception 1
    "d_other_held": dict(steps=[
        prime(A), hot(A),
        dict(clock=(11500, 501), frames=[syn(A, 40000), udp_packet(S, B, 7, 9), reply(A, 40000)],
             want=[(P24, "", HOLD), (ADROP, "", OK), (AFW, "FN", OK)], flows=1,
             records={(A, 13, 1, 3, 11000, 11500, 601), (S, 40000, 1, 0, 11500, 11500, 0)})]),
    # e. flow-pool room 1: A creates; B's SYN passes the detector (first create, OK) and the ACL, FlowAdd finds the pool
    # empty (flow.c:124-129): FLOW_NOMEM, with B's record stepped; the same SYN again: same port, OK, NOMEM again
    "e_room_one": dict(flow_capacity=1, steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000), syn(B, 40000), syn(B, 40000)],
             want=[(AFW, "FN", OK), (FNOMEM, "", OK), (FNOMEM, "", OK)], flows=1,
             records={(A, 80, 0, 0, 10000, 10000, 0), (B, 80, 0, 0, 10000, 10000, 0)})]),
    # e'. with the first creator held instead, the second one creates and its repeat is found
    "e_room_one_first_held": dict(flow_capacity=1, steps=[
        prime(A), hot(A),
        dict(clock=(11500, 501), frames=[syn(A, 40000), syn(B, 40000), syn(B, 40000)],
             want=[(P24, "", HOLD), (AFW, "FN", OK), (AFW, "F", None)], flows=1)]),
    # f. record pool 1.  Two flows exist without records (created with the detector off).  A's packet is found and takes
    # no record, so B's SYN of a new tuple gets the one record (dp_portscan.c:254-266)
    "f_record_for_the_miss": dict(ps_capacity=1, steps=[
        dict(clock=(10000, 500), able=0, frames=[syn(A, 40000), syn(B, 40000)], want=[(AFW, "FN", None)] * 2),
        dict(clock=(10000, 500), frames=[syn(A, 40000, ACK), syn(B, 40001)], want=[(AFW, "F", None), (AFW, "FN", OK)],
             flows=3, records={(B, 80, 0, 0, 10000, 10000, 0)})]),
    # f'. A misses first and takes the record: every miss of B is NOMEM (:256-261): 24, while B's packet of a live flow
    # passes
    "f_record_taken": dict(ps_capacity=1, steps=[
        dict(clock=(10000, 500), able=0, frames=[syn(A, 40000), syn(B, 40000)], want=[(AFW, "FN", None)] * 2),
        dict(clock=(10000, 500), frames=[syn(A, 40002), syn(B, 40001), syn(B, 40000, ACK), syn(B, 40003)],
             want=[(AFW, "FN", OK), (P24, "", NOMEM), (AFW, "F", None), (P24, "", NOMEM)], flows=3,
             records={(A, 80, 0, 0, 10000, 10000, 0)})]),
    # g. a hold released by a rising ts inside the batch (hold 601): ts 599 and 600: HOLD; ts 601: the hold is over, the
    # last branch (14500 - 11000 >= 2 rate), OK, the ACL forwards: created; the fourth packet finds the flow
    "g_hold_released_in_batch": dict(steps=[
        prime(A), hot(A),
        dict(clock=(14500, 502), ts=[599, 600, 601, 601], frames=[syn(A, 40000)] * 4,
             want=[(P24, "", HOLD), (P24, "", HOLD), (AFW, "FN", OK), (AFW, "F", None)], flows=1,
             records={(A, 80, 1, 0, 14500, 14500, 0)})]),
    # h. a non-SYN miss with syn_check 1: FLOW_TCP_NO_SYN_FIRST, the detector is not called (flow.c:204-214): no record
    "h_syn_check_on": dict(steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000, ACK)], want=[(NOSYN, "", None)], flows=0, records=set())]),
    # h'. with syn_check 0 the same packet reaches the detector (a record) and creates the flow
    "h_syn_check_off": dict(syn_check=0, steps=[
        dict(clock=(10000, 500), frames=[syn(A, 40000, ACK)], want=[(AFW, "FN", OK)], flows=1,
             records={(A, 80, 0, 0, 10000, 10000, 0)})]),
    # i. action 1: the state runs, nothing is dropped by the detector: the hot packet is DETECTED and goes on to the ACL
    # (no rule: ACL_DROP); the held source's SYN is HOLD and creates its flow
    "i_action_forward": dict(action=1, steps=[
        prime(A), hot(A, action=1),
        dict(clock=(11500, 501), frames=[syn(A, 40000)], want=[(AFW, "FN", HOLD)], flows=1, drop=0,
             records={(A, 13, 1, 3, 11000, 11500, 601)})]),
}


def kat_model(k):
    o = pyoracle.Oracle(kat_rules(), default_action=DROP)
    ps = psm.PortScanModel(able=1, action=k.get("action", 0), exception_freq=3, hold_seconds=100,
                           capacity=k.get("ps_capacity", 100), cycles_per_second=RATE)
    return o, fpm.FlowPortScanModel(o, k.get("flow_capacity", 100), ps)


def check_step(step, got, what):
    """The step's stated answers against a result (the model's, or a GPU's)."""
    have = [(int(v) & 0xFF, (int(v) >> 16) & fpm.FLOWBITS) for v in got["verdict"]]
    assert have == [(st, BITS[b]) for st, b, _ in step["want"]], what
    for (st, _, _), v, h in zip(step["want"], got["verdict"], got["acl_hit"]):
        if st == P24:  # DROP, no ACL hit, PPE_F_ACL clear
            assert (int(v) >> 8) & 0xFF == abi.ACT_DROP and int(h) == -1 and not (int(v) >> 16) & abi.F_ACL, what


@pytest.mark.parametrize("name", sorted(KATS))
def test_known_answers(name):
    k = KATS[name]
    o, m = kat_model(k)
    for j, step in enumerate(k["steps"]):
        m.ps.able = step.get("able", 1)
        m.ps.clock(*step["clock"])
        hdr, lens = stack(step["frames"])
        ts = np.array(step["ts"], np.uint64) if "ts" in step else None
        got = m.classify_batch(hdr, lens, ts, cfg=o.cfg(0, k.get("syn_check", 1), step["clock"][1]))
        check_step(step, got, (name, j))
        assert got["results"].tolist() == [-1 if r is None else r for _, _, r in step["want"]], (name, j)
        if "flows" in step:
            assert len(m.flows) == step["flows"], (name, j)
        if "records" in step:
            assert m.ps.records() == step["records"], (name, j)
        if "drop" in step:
            assert m.ps.counts["drop"] == step["drop"], (name, j)


def test_detector_off_equals_the_oracle_flow_table():
    """able = 0: the model is pyoracle.OracleFlow over the same batches, rows, counters and table, with a pool small
    enough to run out and aging in between."""
    seq, par = generated()
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)
    m = fpm.FlowPortScanModel(o, par["flow_capacity"], psm.PortScanModel(able=0))
    ft = pyoracle.OracleFlow(o, capacity=par["flow_capacity"])
    nomem = 0
    for b, s in enumerate(seq[:120]):
        for syn_check in ((1, 0) if b % 7 == 3 else (1,)):
            cfg = o.cfg(0, syn_check, s["now_s"])
            got, ref = m.classify_batch(s["hdr"], s["lens"], s["ts"], cfg), ft.classify_batch(s["hdr"], s["lens"], cfg=cfg)
            for key in ("verdict", "flow_hash", "acl_hit", "tuple", "counters"):
                assert np.array_equal(got[key], ref[key]), (b, key)
            nomem += int(((ref["verdict"] & 0xFF) == FNOMEM).sum())
        if s["age"]:
            assert m.age(s["now_s"], 2) == ft.age(s["now_s"], 2)
        d = ft.dump()
        cols = ("sip", "dip", "sport", "dport", "protocol", "pktcnts2d", "pktcntd2s", "bytecnts2d", "bytecntd2s",
                "last_seen")
        assert m.table() == sorted(tuple(int(x) for x in r) for r in zip(*(d[c] for c in cols))), b
        assert m.stats() == ft.stats(), b
    assert nomem > 10 and m.del_flow > 10 and not m.ps.table
    ft.close()


def test_no_flow_ever_equals_the_stateless_detector():
    """A rule set that forwards nothing: no flow is ever created, every L4 packet past syn_check is a miss at the
    detector: PortScanModel.expected over the stateless oracle."""
    seq, par = generated()
    o = pyoracle.Oracle(np.zeros(0, abi.RULE_DTYPE), default_action=DROP)
    mk = lambda: psm.PortScanModel(1, 0, par["freq"], par["hold"], par["ps_capacity"], par["rate"])  # noqa: E731
    m, ref_ps = fpm.FlowPortScanModel(o, par["flow_capacity"], mk()), mk()
    for b, s in enumerate(seq[:120]):
        for p in (m.ps, ref_ps):
            p.clock(s["now_c"], s["now_s"])
        cfg = o.cfg(0, 1, s["now_s"])
        got = m.classify_batch(s["hdr"], s["lens"], s["ts"], cfg)
        want = ref_ps.expected(o.classify_batch(s["hdr"], s["lens"], cfg=cfg), s["hdr"], ts=s["ts"])
        for key in ("verdict", "flow_hash", "acl_hit", "tuple", "results"):
            assert np.array_equal(got[key], want[key]), (b, key)
        assert dict(zip(abi.COUNTERS, (int(x) for x in got["counters"]))) == want["counters"], b
        if s["age"]:
            assert m.ps.timeout(s["now_c"]) == ref_ps.timeout(s["now_c"])
        assert m.ps.records() == ref_ps.records() and m.ps.info() == ref_ps.info(), b
    assert not m.flows and m.ps.counts["drop"] > 100


# ---- the generated sequence of the GPU tests ----
SEED, BATCHES = 20261, 200
_cache = {}


def generated(max_n=None):
    """fpm.gen_sequence at the GPU tests' seed (computed once per size and shared)."""
    max_n = max_n or 1024
    if max_n not in _cache:
        _cache[max_n] = fpm.gen_sequence(SEED, BATCHES, max_n)
    return _cache[max_n]


def run_generated(seq, par, syn_check=1):
    """The model over the sequence: per batch its result; the model itself."""
    o = pyoracle.Oracle(fpm.gen_rules(), default_action=DROP)
    ps = psm.PortScanModel(1, 0, par["freq"], par["hold"], par["ps_capacity"], par["rate"])
    m = fpm.FlowPortScanModel(o, par["flow_capacity"], ps)
    outs = []
    for s in seq:
        ps.clock(s["now_c"], s["now_s"])
        outs.append(m.classify_batch(s["hdr"], s["lens"], s["ts"], o.cfg(0, syn_check, s["now_s"])))
        if s["age"]:
            m.age(s["now_s"], 2)
            ps.timeout(s["now_c"])
    return outs, m


NEEDED = ("ok", "nomem", "detected", "hold", "creator_not_lowest", "creatorless_claim", "nomem_after_ok",
          "found_of_held_source")


def test_generated_sequence_holds_every_case():
    """A condition on the inputs, from the model alone: each case the kernel's resolve phase exists for occurs at least
    10 times over the generated sequence."""
    seq, par = generated()
    _, m = run_generated(seq, par)
    assert all(m.events[k] >= 10 for k in NEEDED), {k: m.events[k] for k in NEEDED}
    branches = set()
    for s0, s1 in zip(seq, seq[1:]):
        d = s1["now_c"] - s0["now_c"]
        branches.add(0 if d < par["rate"] else 1 if d < 2 * par["rate"] else 2)
    assert branches == {0, 1, 2} and m.del_flow >= 10 and m.ps.counts["del_pcb"] >= 1


def test_frozen_scenario():
    """One generated scenario frozen as model output (tests/golden/flow_portscan_v1.npz, written by
    tests/golden/gen_flow_portscan_golden.py): the model, the generator and the oracle under it have not moved."""
    g = np.load(GOLDEN)
    seq, par = fpm.gen_sequence(int(g["seed"]), int(g["batches"]), int(g["max_n"]))
    outs, m = run_generated(seq, par)
    assert np.array_equal(np.concatenate([o["verdict"] for o in outs]), g["verdict"])
    assert np.array_equal(np.concatenate([o["acl_hit"] for o in outs]), g["acl_hit"])
    assert np.array_equal(np.concatenate([o["results"] for o in outs]), g["results"])
    assert np.array_equal(sum(o["counters"] for o in outs), g["counters"])
    assert np.array_equal(np.array(m.table(), np.uint64).reshape(-1, 10), g["flows"])
    assert np.array_equal(np.array(sorted(m.ps.records()), np.uint64).reshape(-1, 7), g["records"])
