"""ppe_flow_stream_portscan on the GPU: the flow kernel with the port-scan detector inside and the TCP session machine
behind it, without the attack monitors (ppe_flow_launch_info kind 7) and with them (kind 8), against
tests/flow_stream_portscan_model.py after every batch, tick and aging step: every output and list layout with its guard
entries, the 32 counters, the 58 stream counters, ppe_attack_info, ppe_portscan_info and its dump, ppe_flow_info, the flow
dump and the session dump with the port byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import stream_session_corpus as sc  # noqa: E402
import test_flow_combined_model as tcm  # noqa: E402
import test_flow_stream_portscan_model as tsp  # noqa: E402
from pktbuild import tcp_packet  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from stream_session_corpus import A, P, c  # noqa: E402
from test_gpu_attack import DEV, PART, PART8, PLAIN, SEP, alloc, collect, compare, to_dev  # noqa: E402
from test_gpu_flow import table  # noqa: E402

LAYOUTS = (SEP, PART, PART8, PLAIN)
PS_INFO = ("live", "new_pcb", "del_pcb", "ok", "nomem", "detected", "hold", "drop")
P24, AFW, FNOMEM = tsp.P24, tsp.AFW, tsp.FNOMEM
KINDS = pytest.mark.parametrize("kind", [7, 8], ids=["kind7", "kind8"])


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    yield e
    for x in e:
        x.close()


@pytest.fixture(scope="module")
def MAX(engines):
    return min(engines[0].flow_portscan_max(), engines[0].flow_stream_max())


class Rig(tsp.Kat):
    """An engine with sessions attached, a port-scan table flow-attached, for kind 8 the monitors flow-attached and both
    pair switches on, and ppe_flow_stream_portscan on; the model beside it (tests/test_flow_stream_portscan_model.py's
    Kat: the known answers run on a Rig as they run on the model).  step() runs one batch through both and compares
    everything."""

    def __init__(self, eng, kind, switch=1, sessions=True, table=True, monitors=None, combine=1, st_monitors=1,
                 max_batch=2048, ps_max_batch=2048, tune=None, outs=None, **kw):
        super().__init__(kind, **kw)
        self.eng, self.outs_cycle, self.nstep = eng, outs, 0
        monitors = kind == 8 if monitors is None else monitors
        if tune:
            eng.tuning(**tune)
        mod = self.mod
        rules = kw.get("rules")
        eng.commit(tsp.kat_rules() if rules is None else rules, default_action=kw.get("default", tsp.DROP))
        eng.flow_create(mod.fp.capacity, max_batch)
        eng.stream_tcp(track=1 if sessions else 0, reasm=0)
        if sessions:
            eng.flow_stream(1)
        eng.flow_stream_portscan(switch)
        eng.flow_combine(combine if monitors else 0)
        eng.flow_stream_monitors(st_monitors if monitors else 0)
        eng.clear_counters()
        eng.clear_stream_track_counters()
        ps = mod.fp.ps
        self.ps = eng.portscan(attach="flow", able=ps.able, action=ps.action, exception_freq=ps.freq,
                               hold_seconds=ps.hold_seconds, capacity=ps.capacity, max_batch=ps_max_batch,
                               cycles_per_second=ps.rate) if table else None
        self.atk = eng.attack(mod.atk.cfg(), attach="flow") if monitors else None
        self.sessions, self.monitors = sessions, monitors
        self.counters = np.zeros(32, np.int64)
        self.keep = []

    def close(self):
        if self.atk is not None:
            self.atk.close()
        if self.ps is not None:
            self.ps.close()
        e = self.eng
        e.flow_stream_portscan(0)
        e.flow_stream_monitors(0)
        e.flow_combine(0)
        e.flow_destroy()
        e.stream_tcp(track=0)

    def clock(self, cycles, seconds):
        super().clock(cycles, seconds)
        if self.ps is not None:
            self.ps.clock(cycles, seconds)
        if self.atk is not None:
            self.atk.clock(seconds)

    def tick(self, now, check=True):
        super().tick(now)
        self.atk.tick(now)
        if check:
            self.same("after a tick")

    def set_rules(self, pd=None, td=None, hold=600):
        super().set_rules(pd, td, hold)
        self.atk.set(self.mod.atk.cfg())

    def age(self, now, timeout, cycles=None):
        n = self.mod.age(now, timeout)
        assert self.eng.flow_age(now, timeout) == n
        if cycles is not None:
            assert self.ps.age(cycles) == self.mod.fp.ps.timeout(cycles)
        self.same("after aging")
        return n

    def enqueue(self, hdr, lens, ports, ts, outs, syn_check=1):
        th, tl, tp = to_dev(hdr, lens, ports if self.monitors else None)
        if self.atk is not None:
            self.atk.ports([tp] if tp is not None else None)
        tts = torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to(DEV) if ts is not None else None
        out = alloc(len(lens), outs)
        self.eng.classify_flow_torch(th, tl, out, cfg=self.eng.cfg(0, syn_check, self.now), ts=tts)
        self.keep = [(th, tl, tp, tts)]
        return out

    def run(self, hdr, lens, ports=None, ts=None, outs=SEP, syn_check=1, what="", launch=None):
        n = len(lens)
        out = self.enqueue(hdr, lens, ports, ts, outs, syn_check)
        torch.cuda.synchronize()
        exp, reasons = self.mod.classify_batch(hdr, lens, ports, ts, self.mod.o.cfg(0, syn_check, self.now))
        self.counters += exp["counters"].astype(np.int64)
        compare(collect(out, n), exp, n, what)
        assert self.eng.flow_launch_info() == (launch or (self.kind, 1)), what
        self.same(what)
        self.out = exp
        return exp, reasons

    def step(self, items, ports=None, ts=None, syn_check=1):
        """Kat.step on both sides (the known answers call this)."""
        hdr, lens = tsp.stack(items)
        outs = LAYOUTS[self.nstep % 4] if self.outs_cycle is None else self.outs_cycle
        self.nstep += 1
        exp, r = self.run(hdr, lens, None if ports is None else np.array(ports, np.uint8),
                          None if ts is None else np.array(ts, np.uint64), outs, syn_check, f"step {self.nstep}")
        return (exp["verdict"] & 0xFF).tolist(), exp["results"].tolist(), r.tolist()

    def same(self, what=""):
        e, mod = self.eng, self.mod
        cnt = e.counters()
        assert [cnt[k] for k in abi.COUNTERS] == self.counters[:len(abi.COUNTERS)].tolist(), what
        assert list(e.stream_track_counters().values()) == mod.cnt.c, what
        assert table(e.flow_dump()) == mod.table(), what
        fi, st = e.flow_info(), mod.stats()
        assert (fi["live"], fi["new_flow"], fi["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"]), what
        if self.ps is not None:
            pi, mi = self.ps.info(), mod.fp.ps.info()
            assert {k: pi[k] for k in PS_INFO} == {k: mi[k] for k in PS_INFO}, what
            assert fpm.ps_records(self.ps.dump()) == mod.fp.ps.records(), what
        if self.atk is not None:
            info, want = self.atk.info(), mod.atk.info()
            for p in range(4):
                g = {k: info["ai"][p][k] for k in abi.ATTACK_STATE_FIELDS}
                assert g == want["ai"][p], (what, "port", p, g, want["ai"][p])
            assert {k: info[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}, what
        if self.sessions:
            got = {tuple(sorted(((x.sip, x.sport), (x.dip, x.dport)))):
                   (x.state, x.flags) + x.client.astuple() + x.server.astuple() + (x.pad,) for x in e.flow_stream_dump()}
            want = mod.sessions()
            assert got == want, (what, [(k, got.get(k), want[k]) for k in want if got.get(k) != want[k]][:3])


def gen_rig(eng, kind, par, **kw):
    return Rig(eng, kind, rules=fpm.gen_rules(), pd=tcm.GEN_PD, td=tcm.GEN_TD, atk_hold=tcm.GEN_HOLD,
               flow_capacity=par["flow_capacity"], ps_capacity=par["ps_capacity"], freq=par["freq"], hold=par["hold"],
               rate=par["rate"], **kw)


def pool(seed, n):
    """n packets of the generated population (three generated batches joined and repeated): hdr, lens, ports."""
    seq, _ = tsp.gen_sequence(seed, 3, 130)
    hdr, lens, ports = (np.concatenate([q[k] for q in seq]) for k in ("hdr", "lens", "ports"))
    reps = -(-n // len(lens))
    return np.tile(hdr, (reps, 1))[:n], np.tile(lens, reps)[:n], np.tile(ports, reps)[:n]


def run_sequence(rig, seq, outs=None):
    for b, q in enumerate(seq):
        if rig.kind == 8 and q["tick"]:
            rig.tick(q["now_s"], check=False)
        rig.clock(q["now_c"], q["now_s"])
        rig.run(q["hdr"], q["lens"], q["ports"], q["ts"], outs or LAYOUTS[b % 4], what=f"batch {b} n={len(q['lens'])}")
        if q["age"]:
            rig.age(q["now_s"], 2, q["now_c"])


@pytest.mark.parametrize("name,kind", tsp.KAT_CASES, ids=[f"{n}-kind{k}" for n, k in tsp.KAT_CASES])
def test_known_answers(engines, name, kind):
    """tests/test_flow_stream_portscan_model.py's hand-derived answers (a)-(h): the stated answers, and everything
    against the model, the four output layouts in turn."""
    case, _, kw = tsp.KATS[name]
    rig = Rig(engines[0], kind, **kw)
    try:
        case(rig)
    finally:
        rig.close()


@KINDS
def test_sizes_and_the_refusal_above_the_maximum(engines, MAX, kind):
    """n in {1, 63, 64, 65, MAX - 1, MAX} on one set of tables; MAX + 1 is refused with nothing written and every state
    unchanged."""
    eng = engines[0]
    _, par = tsp.generated()
    rig = gen_rig(eng, kind, par)
    try:
        for k, n in enumerate((1, 63, 64, 65, MAX - 1, MAX, 65)):
            hdr, lens, ports = pool(900 + k, n)
            if kind == 8:
                rig.tick(1000 + k, check=False)
            rig.clock(10_000 + 400 * k, 1000 + k)
            ts = np.sort(1000 + k + np.arange(n) % 3).astype(np.uint64)
            rig.run(hdr, lens, ports, ts, LAYOUTS[k % 4], what=f"n={n}")
        assert rig.mod.fp.ps.counts["drop"] > 0 and sum(rig.mod.cnt.c) > 0
        hdr, lens, ports = pool(990, MAX + 1)
        out = alloc(MAX + 1, SEP)
        th, tl, tp = to_dev(hdr, lens, ports)
        if rig.atk is not None:
            rig.atk.ports([tp])
        with pytest.raises(PPEError, match="-95.*at most"):  # (the batch is what is refused, not the combination)
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, 2000))
        torch.cuda.synchronize()
        for k, v in out.items():
            assert (v.cpu().numpy() == (0xEE if k == "part8" else -7)).all(), k
        rig.same("after the refusal")
    finally:
        rig.close()


@KINDS
def test_one_flows_walk_across_the_tile_boundary_interleaved_with_a_scanners_chain(engines, kind):
    """One connection's packets at indices 0, 2, ..., 126 (a walk across the 63 | 64 boundary) interleaved with one
    scanner's SYNs to changing ports at the odd indices (one source: one resolve round per SYN)."""
    rig = Rig(engines[0], kind, rules=np.zeros(0, abi.RULE_DTYPE), default=tsp.FW, freq=3, hold=100)
    try:
        conv = tsp.script(1, sc.EST + [c(A | P, 1 + 10 * j, 1, plen=10) for j in range(61)])
        x = 0x0A000077
        scan = [tcp_packet(x, tsp.SRV, 40000, 100 + j) for j in range(64)]
        items = [it for pair in zip(conv, scan) for it in pair]
        rig.clock(10000, 500)
        st, res, r = rig.step(items, [j & 3 for j in range(128)])
        assert st == [AFW] * 128 and not any(r) and res[1::2] == [tsp.OK] * 64 and res[2::2] == [-1] * 63
        assert rig.eng.flow_portscan_rounds() >= 64
        assert rig.mod.ssn[tsp.key(1)].client.next_seq == 1001 + 610
        rig.clock(11500, 501)  # the window rolls: the scanner is detected, its next SYNs are held
        st, res, r = rig.step([scan[0], tcp_packet(x, tsp.SRV, 40001, 7), conv[3], tcp_packet(x, tsp.SRV, 40002, 8)])
        assert st == [AFW, P24, 29 if r[2] else AFW, P24] and res == [-1, tsp.DETECTED, -1, tsp.HOLD]
    finally:
        rig.close()


@KINDS
def test_one_flow_owning_65_packets(engines, kind):
    rig = Rig(engines[0], kind)
    try:
        rig.clock(10000, 500)
        st, res, r = rig.step(tsp.script(1, sc.EST + [c(A | P, 1 + 10 * j, 1, plen=10) for j in range(62)]), [1] * 65)
        assert st == [AFW] * 65 and res == [tsp.OK] + [-1] * 64 and not any(r)
        assert rig.mod.ssn[tsp.key(1)].client.next_seq == 1001 + 620
    finally:
        rig.close()


@KINDS
def test_max_sources_against_three_records(engines, MAX, kind):
    """MAX SYNs of MAX sources, three detector records: three flows, the rest status 24 (NOMEM), no session for them."""
    rig = Rig(engines[0], kind, ps_capacity=3, flow_capacity=2000, rules=np.zeros(0, abi.RULE_DTYPE), default=tsp.FW)
    try:
        rig.clock(10000, 500)
        st, res, r = rig.step([it for f in range(1, MAX + 1) for it in tsp.script(f, sc.SYN_SENT)],
                              [f & 3 for f in range(MAX)])
        assert st == [AFW] * 3 + [P24] * (MAX - 3) and res == [tsp.OK] * 3 + [tsp.NOMEM] * (MAX - 3)
        assert len(rig.mod.sessions()) == 3 and rig.stream() == {"SYN_COUNT": 3}
    finally:
        rig.close()


@KINDS
def test_flow_capacity_eight_with_creators_past_it(engines, kind):
    rig = Rig(engines[0], kind, flow_capacity=8)
    try:
        rig.clock(10000, 500)
        items = [it for f in range(1, 21) for it in tsp.script(f, sc.SYN_RECV)]
        st, res, r = rig.step(items, [f & 3 for f in range(40)])
        assert st[:16] == [AFW] * 16 and st[16::2] == [FNOMEM] * 12 and res[16::2] == [tsp.OK] * 12
        assert len(rig.mod.sessions()) == 8 and rig.stream()["SYN_COUNT"] == 8
    finally:
        rig.close()


@KINDS
def test_the_generated_sequence_with_aging_and_a_rehash(engines, kind):
    """tests/test_flow_stream_portscan_model.py's generated sequence (each of (a)-(f) at least 10 times), ticks, both
    tables aged; the flows aged out pass a quarter of the table's slots, so the table rehashes and the session records
    move with their flows."""
    seq, par = tsp.generated()
    rig = gen_rig(engines[0], kind, par, max_batch=256)
    try:
        run_sequence(rig, seq)
        assert rig.eng.flow_info()["rehashes"] >= 1 and rig.mod.fp.del_flow > 64
    finally:
        rig.close()


def test_frozen_scenario(engines):
    g = np.load(tsp.GOLDEN)
    seq, par = tsp.gen_sequence(int(g["seed"]), int(g["batches"]), int(g["max_n"]))
    rig = gen_rig(engines[0], 8, par)
    try:
        run_sequence(rig, seq)
        assert np.array_equal(np.array(rig.mod.table(), np.uint64).reshape(-1, 10), g["flows"])
        assert np.array_equal(np.array(rig.mod.cnt.c, np.uint64), g["stream_counters"])
    finally:
        rig.close()


@pytest.mark.parametrize("nrules,tune,place", [(256, dict(), "lds"), (4096, dict(), "split"),
                                               (256, dict(lds_image=0), "global")], ids=["lds", "split", "global"])
def test_the_three_image_placements(engines, nrules, tune, place):
    """Kind 8 over an image in LDS, split and in global memory (the same rule set sizes and tuning the session kernel's
    tests use), the corpus' conversations behind scanners."""
    eng = engines[1]
    old = eng.tuning()
    try:
        rig = Rig(eng, 8, rules=synth.make_rules(nrules, seed=nrules), default=tsp.FW, tune=tune, pd=tcm.GEN_PD,
                  td=tcm.GEN_TD, atk_hold=1, freq=2, hold=2, ps_capacity=64, flow_capacity=3000)
        try:
            for b, (hdr, lens, ports) in enumerate(tsp.conv_batches()[:3]):
                rig.clock(10_000 + 700 * b, 1000 + b)
                rig.run(hdr, lens, ports, None, LAYOUTS[b % 4], what=f"{place} batch {b}")
        finally:
            rig.close()
    finally:
        eng.tuning(**old)


# ---- the switches ----
def sessions_by_key(eng):
    """ppe_flow_stream_dump as {(sip, dip, sport, dport): the record's fields}: independent of the slot order."""
    return {(x.sip, x.dip, x.sport, x.dport): (x.state, x.flags, x.pad, x.client.astuple(), x.server.astuple())
            for x in eng.flow_stream_dump()}


def outputs_equal(x, y):
    return all(torch.equal(x[k], y[k]) for k in x)


@KINDS
def test_switch_off_refuses_with_nothing_touched_and_toggles_between_batches(engines, kind):
    eng = engines[0]
    _, par = tsp.generated()
    seq, _ = tsp.gen_sequence(31, 4, 100)
    rig = gen_rig(eng, kind, par, switch=0)
    try:
        for b, q in enumerate(seq):
            rig.clock(q["now_c"], q["now_s"])
            eng.flow_stream_portscan(0)
            out = alloc(len(q["lens"]), SEP)
            th, tl, tp = to_dev(q["hdr"], q["lens"], q["ports"] if kind == 8 else None)
            if rig.atk is not None:
                rig.atk.ports([tp])
            with pytest.raises(PPEError, match="-95.*port-scan table or attack monitors"):  # (the text it always had)
                eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, q["now_s"]))
            torch.cuda.synchronize()
            for k, v in out.items():
                assert (v.cpu().numpy() == -7).all(), k
            rig.same(f"after the refusal {b}")
            eng.flow_stream_portscan(1)
            rig.run(q["hdr"], q["lens"], q["ports"], q["ts"], what=f"batch {b}")
        with pytest.raises(PPEError, match="-22"):
            eng.flow_stream_portscan(2)
    finally:
        rig.close()


def test_kind_8_is_refused_when_either_pair_switch_is_off(engines):
    eng = engines[0]
    _, par = tsp.generated()
    seq, _ = tsp.gen_sequence(33, 1, 64)
    q = seq[0]
    for combine, st_monitors in ((0, 1), (1, 0), (0, 0)):
        rig = gen_rig(eng, 8, par, combine=combine, st_monitors=st_monitors)
        try:
            rig.clock(q["now_c"], q["now_s"])
            out = alloc(len(q["lens"]), SEP)
            th, tl, tp = to_dev(q["hdr"], q["lens"], q["ports"])
            rig.atk.ports([tp])
            with pytest.raises(PPEError, match="-95"):
                eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, q["now_s"]))
            torch.cuda.synchronize()
            for k, v in out.items():
                assert (v.cpu().numpy() == -7).all(), k
            rig.same("after the refusal")
            eng.flow_combine(1)
            eng.flow_stream_monitors(1)
            rig.run(q["hdr"], q["lens"], q["ports"], q["ts"], what="both on")
        finally:
            rig.close()


@pytest.mark.parametrize("what", ["able0_kind5", "able0_kind6", "only_sessions", "only_table"])
def test_switch_on_outside_the_combination_is_byte_identical_to_a_twin(engines, what):
    """Switch 1 with able = 0 (kinds 5 / 6 run), with only sessions or only the table attached: every output byte, counter
    and dump equals a twin context that never called ppe_flow_stream_portscan, given the same calls otherwise.  (With
    able = 0 and the switch off the twin would refuse: it runs without a table instead, which the planner says is the same.)"""
    _, par = tsp.generated()
    seq, _ = tsp.gen_sequence(35, 3, 120)
    kind = 8 if what == "able0_kind6" else 7
    kw = dict(sessions=what != "only_table", max_batch=256)
    a = gen_rig(engines[0], kind, par, switch=1, able=0 if what.startswith("able0") else 1,
                table=what != "only_sessions", **kw)
    b = gen_rig(engines[1], kind, par, switch=0, able=0 if what.startswith("able0") else 1,
                table=what == "only_table", **kw)
    want = {"able0_kind5": (5, 1), "able0_kind6": (6, 1), "only_sessions": (5, 1), "only_table": (2, 1)}[what]
    try:
        for j, q in enumerate(seq):
            outs = []
            for rig in (a, b):
                rig.clock(q["now_c"], q["now_s"])
                outs.append(rig.enqueue(q["hdr"], q["lens"], q["ports"], q["ts"], LAYOUTS[j % 4]))
            torch.cuda.synchronize()
            assert outputs_equal(*outs), (what, j)
            assert a.eng.flow_launch_info() == b.eng.flow_launch_info() == want
            assert a.eng.counters() == b.eng.counters()
            assert a.eng.stream_track_counters() == b.eng.stream_track_counters()
            assert table(a.eng.flow_dump()) == table(b.eng.flow_dump())
            if kw["sessions"]:
                # (by key, not in dump order: which slot of its group a new flow takes is a race among the classify
                # phase's waves, so two flows created in one batch may stand in either order in either table)
                da, db = sessions_by_key(a.eng), sessions_by_key(b.eng)
                assert da == db and len(da) == len(a.eng.flow_stream_dump()), (what, j)
            if kind == 8:
                assert a.atk.info() == b.atk.info()
            if what == "only_table":
                assert fpm.ps_records(a.ps.dump()) == fpm.ps_records(b.ps.dump()) and a.ps.info() == b.ps.info()
    finally:
        a.close()
        b.close()


def test_refusals_leave_everything(engines, MAX):
    """reasm / midstream / async_oneside 1 (PPE_ENOTSUP), a stride under 144 B and n above the port-scan table's max_batch
    (PPE_EINVAL): nothing written, nothing moved."""
    eng = engines[0]
    _, par = tsp.generated()
    hdr, lens, _ = pool(37, 100)
    q = dict(hdr=hdr, lens=lens, ts=np.full(100, 1000, np.uint64), now_s=1000)
    rig = gen_rig(eng, 7, par, ps_max_batch=64)
    try:
        rig.clock(10_000, 1000)

        def refused(hdr, lens, code):
            out = alloc(len(lens), SEP)
            th, tl, _ = to_dev(hdr, lens)
            with pytest.raises(PPEError, match=code):
                eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, q["now_s"]))
            torch.cuda.synchronize()
            for k, v in out.items():
                assert (v.cpu().numpy() == -7).all(), k
            rig.same("after a refusal")

        for mode in (dict(midstream=1), dict(async_oneside=1), dict(reasm=1)):
            eng.stream_tcp(track=1, **mode)
            refused(q["hdr"], q["lens"], "-95")
            eng.stream_tcp(track=1, reasm=0)
        refused(np.ascontiguousarray(q["hdr"][:, :128]), q["lens"], "-22")
        refused(q["hdr"][:65], q["lens"][:65], "-22.*max_batch")
        rig.run(q["hdr"][:64], q["lens"][:64], None, q["ts"][:64], what="n = the table's max_batch")
    finally:
        rig.close()
