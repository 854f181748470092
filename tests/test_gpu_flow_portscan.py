"""The port-scan detector on the flow-table path (ppe_flow_portscan_attach, csrc/ppe_kernels_flow_portscan.hip): an engine
with a flow table and a port-scan table flow-attached, the serial model beside it (tests/flow_portscan_model.py).  After
every batch the verdict, flow hash, ACL hit, tuple and compacted lists, the 32 counters, ppe_flow_info and the whole
ppe_flow_dump, ppe_portscan_info and the whole ppe_portscan_dump must equal the model's, with the 64 guard entries behind
every output untouched.  Integer work: no tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import flow_portscan_model as fpm  # noqa: E402
import portscan_model as psm  # noqa: E402
import pyoracle  # noqa: E402
import test_flow_portscan_model as tm  # noqa: E402
from pktbuild import tcp_packet, udp_packet  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402
from test_gpu_attack import DEV, PART, PART8, PLAIN, SEP, alloc, collect, compare, to_dev  # noqa: E402
from test_gpu_flow import table  # noqa: E402

LAYOUTS = (SEP, PART, PART8, PLAIN)  # (the flow path has no packed layout)
FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP
PS_INFO = ("live", "new_pcb", "del_pcb", "ok", "nomem", "detected", "hold", "drop")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def MAX(eng):
    return eng.flow_portscan_max()


class Rig:
    """An engine with a flow table and a port-scan table flow-attached, and the model: step() runs one batch through both
    and compares everything."""

    def __init__(self, eng, rules, default_action=DROP, flow_capacity=100, ps_capacity=100, freq=3, hold=100, action=0,
                 rate=1000, syn_check=1, max_batch=1 << 14, ps_max_batch=2048, commit=True, attach=True):
        self.eng, self.syn_check = eng, syn_check
        if commit:
            eng.commit(rules, default_action=default_action)
        eng.flow_create(flow_capacity, max_batch)
        eng.clear_counters()
        self.o = pyoracle.Oracle(rules, default_action=default_action)
        self.m = fpm.FlowPortScanModel(self.o, flow_capacity, psm.PortScanModel(1, action, freq, hold, ps_capacity, rate))
        self.ps = eng.portscan(attach="flow" if attach else False, able=1, action=action, exception_freq=freq,
                               hold_seconds=hold, capacity=ps_capacity, max_batch=ps_max_batch, cycles_per_second=rate)
        self.counters = np.zeros(32, np.uint64)
        self.now = 0

    def close(self):
        self.ps.close()
        self.eng.flow_destroy()

    def clock(self, cycles, seconds):
        self.ps.clock(cycles, seconds)
        self.m.ps.clock(cycles, seconds)
        self.now = seconds

    def able(self, v):
        self.ps.set(able=v)
        self.m.ps.able = v

    def enqueue(self, hdr, lens, ts=None, outs=SEP, syn_check=None):
        th, tl, _ = to_dev(hdr, lens)
        tts = torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to(DEV) if ts is not None else None
        out = alloc(len(lens), outs)
        sc = self.syn_check if syn_check is None else syn_check
        self.eng.classify_flow_torch(th, tl, out, cfg=self.eng.cfg(0, sc, self.now), ts=tts)
        return out, (th, tl, tts), self.o.cfg(0, sc, self.now)

    def check(self, out, hdr, lens, ts, cfg, what=""):
        n = len(lens)
        ref = self.m.classify_batch(hdr, lens, ts, cfg)
        got = collect(out, n)
        compare(got, ref, n, what)
        self.counters += ref["counters"]
        return got, ref

    def step(self, hdr, lens, ts=None, outs=SEP, syn_check=None, what=""):
        out, keep, cfg = self.enqueue(hdr, lens, ts, outs, syn_check)
        torch.cuda.synchronize()
        got, ref = self.check(out, hdr, lens, ts, cfg, what)
        assert self.eng.flow_launch_info() == ((2, 1) if self.m.ps.able == 1 else self.plain_kind(len(lens))), what
        self.same(what)
        return got, ref

    def plain_kind(self, n):
        return (1, 1) if self.eng.lib.ppe_pick_flow_small(n, 1, 0) else (0, 2)

    def same(self, what=""):
        cnt = self.eng.counters()
        assert [cnt[c] for c in abi.COUNTERS] == self.counters[:len(abi.COUNTERS)].tolist(), what
        assert table(self.eng.flow_dump()) == self.m.table(), what
        info, st = self.eng.flow_info(), self.m.stats()
        assert (info["live"], info["new_flow"], info["del_flow"]) == (st["live"], st["new_flow"], st["del_flow"]), what
        pi, mi = self.ps.info(), self.m.ps.info()
        assert {k: pi[k] for k in PS_INFO} == {k: mi[k] for k in PS_INFO}, what
        assert fpm.ps_records(self.ps.dump()) == self.m.ps.records(), what

    def age(self, now_s, now_c, timeout=2):
        assert self.eng.flow_age(now_s, timeout) == self.m.age(now_s, timeout)
        assert self.ps.age(now_c) == self.m.ps.timeout(now_c)
        self.same("after aging")


@pytest.mark.parametrize("name", sorted(tm.KATS))
def test_known_answers(eng, name):
    """tests/test_flow_portscan_model.py's hand-derived answers a-i, against the stated answers and the model."""
    k = tm.KATS[name]
    rig = Rig(eng, tm.kat_rules(), flow_capacity=k.get("flow_capacity", 100), ps_capacity=k.get("ps_capacity", 100),
              action=k.get("action", 0), syn_check=k.get("syn_check", 1))
    try:
        for j, step in enumerate(k["steps"]):
            rig.able(step.get("able", 1))
            rig.clock(*step["clock"])
            hdr, lens = tm.stack(step["frames"])
            ts = np.array(step["ts"], np.uint64) if "ts" in step else None
            got, ref = rig.step(hdr, lens, ts, outs=LAYOUTS[j % 4], what=f"{name} step {j}")
            tm.check_step(step, got, (name, j))
            assert ref["results"].tolist() == [-1 if r is None else r for _, _, r in step["want"]]
            if "flows" in step:
                assert rig.eng.flow_info()["live"] == step["flows"]
            if "records" in step:
                assert fpm.ps_records(rig.ps.dump()) == step["records"]
            if "drop" in step:
                assert rig.ps.info()["drop"] == step["drop"]
        if name == "a_held_twice":  # the twice-dropped tuple's claimed slot went back as a tombstone, then one more claim
            assert rig.eng.flow_info()["tombstones"] >= 1
    finally:
        rig.close()


def gen_rig(eng, par, **kw):
    return Rig(eng, fpm.gen_rules(), flow_capacity=par["flow_capacity"], ps_capacity=par["ps_capacity"], freq=par["freq"],
               hold=par["hold"], rate=par["rate"], **kw)


def test_sizes_and_the_refusal_above_the_maximum(eng, MAX):
    """n in {1, 63, 64, 65, MAX - 1, MAX} on one pair of tables; MAX + 1 is refused with nothing written and both tables
    unchanged."""
    _, par = tm.generated()
    rig = gen_rig(eng, par)
    rng = np.random.default_rng(11)
    try:
        for k, n in enumerate((1, 63, 64, 65, MAX - 1, MAX, 65, 1)):
            rig.clock(10_000 + 400 * k, 1000 + k)
            hdr, lens = fpm.gen_batch(rng, n)
            rig.step(hdr, lens, (1000 + k + rng.integers(0, 3, n)).astype(np.uint64), outs=LAYOUTS[k % 4], what=f"n={n}")
        hdr, lens = fpm.gen_batch(rng, MAX + 1)
        th, tl, _ = to_dev(hdr, lens)
        out = alloc(MAX + 1, SEP)
        with pytest.raises(PPEError, match="-95"):
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, 2000))
        torch.cuda.synchronize()
        for k, v in out.items():
            assert (v.cpu().numpy() == -7).all(), k
        rig.same("after the refusal")
        rig.able(0)  # the detector off: the same batch through today's kernels, the table still flow-attached
        rig.step(hdr, lens, what="able 0 above the maximum")
    finally:
        rig.close()


@pytest.mark.parametrize("hot", [False, True], ids=["quiet", "hot"])
def test_one_scanner_owns_the_batch(eng, MAX, hot):
    """One source, a new port with every packet, batches of 1, 64, 65 and MAX.  After a quiet window every packet is OK
    and creates its flow; after a hot one (last_exception >= freq once the window rolls) the first change is DETECTED
    and the rest HOLD."""
    rules = np.zeros(1, abi.RULE_DTYPE)
    rules["sport_end"] = rules["dport_end"] = 65535
    rules["protocol_end"] = 255
    rules["action"] = FW
    for j, n in enumerate((1, 64, 65, MAX)):
        rig = Rig(eng, rules, flow_capacity=4096, freq=3, hold=100)
        try:
            src = 0x0A000001
            rig.clock(10_000, 500)
            prime = [udp_packet(src, 0x0B000001, 5000, 100 + p) for p in range(5 if hot else 1)]
            rig.step(*tm.stack(prime), what="prime")
            rig.clock(11_500, 501)  # the window rolls at the batch's first packet
            frames = [tcp_packet(src, 0x0B000001, 40000, 1000 + p, flags=0x02) for p in range(n)]
            got, ref = rig.step(*tm.stack(frames), outs=LAYOUTS[j % 4], what=f"scanner n={n} hot={hot}")
            st = (got["verdict"] & 0xFF).tolist()
            if hot:
                assert st == [ST["PORTSCAN_DROP"]] * n and ref["results"].tolist() == [psm.DETECTED] + [psm.HOLD] * (n - 1)
                assert rig.eng.flow_info()["live"] == len(prime)
            else:
                assert st == [ST["ACL_FW"]] * n and rig.eng.flow_info()["live"] == n + 1
        finally:
            rig.close()


def test_max_distinct_sources_against_three_records(eng, MAX):
    rules = np.zeros(0, abi.RULE_DTYPE)
    rig = Rig(eng, rules, default_action=FW, flow_capacity=4096, ps_capacity=3)
    try:
        rig.clock(10_000, 500)
        frames = [udp_packet(0x0A000001 + i, 0x0B000001, 5000, 53) for i in range(MAX)]
        got, ref = rig.step(*tm.stack(frames), what="MAX sources")
        assert ref["results"].tolist() == [psm.OK] * 3 + [psm.NOMEM] * (MAX - 3)
        assert rig.ps.info()["live"] == 3 and rig.eng.flow_info()["live"] == 3
        got, ref = rig.step(*tm.stack(frames[::-1]), outs=PART, what="again, reversed")  # three found, the rest NOMEM
        assert (ref["results"] == psm.NOMEM).sum() == MAX - 3 and (ref["results"] == -1).sum() == 3
    finally:
        rig.close()


def test_two_hundred_generated_batches(eng, MAX):
    """tests/test_flow_portscan_model.py's generated sequence (every case of the resolve phase at least 10 times, by
    test_generated_sequence_holds_every_case): random sizes 1..MAX, both tables aged in between, and flow rehashes in
    between, brought about by the tombstones of creator-less claims and of the aging (a table of 4,096 slots rehashes
    above 1,024 tombstones; the library has no call that forces one)."""
    assert MAX == 1024 or pytest.fail("the generated sequence is sized for PPE_FLOW_PS_MAX = 1024")
    seq, par = tm.generated()
    rig = gen_rig(eng, par, max_batch=1024, ps_max_batch=1024)
    try:
        for b, s in enumerate(seq):
            rig.clock(s["now_c"], s["now_s"])
            out, keep, cfg = rig.enqueue(s["hdr"], s["lens"], s["ts"], LAYOUTS[b % 4])
            torch.cuda.synchronize()
            rig.check(out, s["hdr"], s["lens"], s["ts"], cfg, f"batch {b}")
            rig.same(f"batch {b}")
            if s["age"]:
                rig.age(s["now_s"], s["now_c"])
        assert rig.eng.flow_info()["rehashes"] >= 1
        assert all(rig.m.events[k] >= 10 for k in tm.NEEDED)
    finally:
        rig.close()


@pytest.mark.parametrize("nrules,tune,image", [(64, dict(), "lds"), (4096, dict(), "split"),
                                               (64, dict(lds_image=0), "global")], ids=["lds", "split", "global"])
def test_each_image_placement(eng, MAX, nrules, tune, image):
    rules = synth.make_rules(nrules, seed=31)
    old = eng.tuning()
    try:
        eng.commit(rules, default_action=FW)
        eng.tuning(**tune)
        img, tn, p = eng.image(), abi.Tuning(**eng.tuning()), abi.Plan()
        assert eng.lib.ppe_plan_image(img.ctypes.data, len(img), C.byref(tn), 1, C.byref(p)) == 0
        assert ("global", "lds", "split")[p.mode] == image, p.as_dict()
        rig = Rig(eng, rules, default_action=FW, flow_capacity=300, ps_capacity=40, freq=2, hold=3, commit=False)
        try:
            for k, n in enumerate((65, MAX - 3, 5, MAX)):
                pk = synth.make_flow_packets(n, rules, n_flows=400, seed=7300 + k, template_seed=7000, kind="udp64",
                                             stride=64, malformed_frac=0.02)
                rig.clock(10_000 + 700 * k, 1000 + k)
                rig.step(pk["hdr"], pk["len"], outs=LAYOUTS[k % 4], what=f"{image} n={n}")
            assert rig.m.ps.counts["drop"] > 0 and rig.m.stats()["live"] > 0
        finally:
            rig.close()
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("outs", LAYOUTS, ids=["sep", "part", "part8", "plain"])
def test_every_list_layout(eng, MAX, outs):
    _, par = tm.generated()
    rig = gen_rig(eng, par)
    rng = np.random.default_rng(17)
    try:
        for k, n in enumerate((MAX, 200, 65)):
            rig.clock(10_000 + 1500 * k, 1000 + k)
            hdr, lens = fpm.gen_batch(rng, n)
            rig.step(hdr, lens, outs=outs, what=f"n={n}")
    finally:
        rig.close()


@pytest.mark.parametrize("n", [64, 8000])
def test_detector_off_or_detached_is_the_plain_flow_path(eng, n):
    """able = 0, and a detached table: byte-identical outputs, counters and flow table to a context that never had one."""
    rules = synth.make_rules(256, seed=21)
    pks = [synth.make_flow_packets(n, rules, n_flows=300, seed=7900 + k, template_seed=7000, kind="udp64", stride=64,
                                   malformed_frac=0.02) for k in range(2)]
    runs = []
    for mode in ("never", "able0", "detached"):
        e = Engine(0)
        try:
            e.commit(rules, default_action=FW)
            e.flow_create(1000, 1 << 14)
            ps = None
            if mode != "never":
                ps = e.portscan(attach="flow", able=1, exception_freq=1, capacity=4, max_batch=2048)
                if mode == "able0":
                    ps.set(able=0)
                else:
                    ps.detach_flow()
            res = []
            for k, pk in enumerate(pks):
                th, tl, _ = to_dev(pk["hdr"], pk["len"])
                out = alloc(n, SEP)
                e.classify_flow_torch(th, tl, out, cfg=e.cfg(0, 1, 1000 + k))
                torch.cuda.synchronize()
                res.append({k2: v.cpu().numpy().tobytes() for k2, v in out.items()})
            assert e.flow_launch_info() == ((1, 1) if n == 64 else (0, 2))
            runs.append((res, e.counters(), table(e.flow_dump())))
            if ps is not None:
                assert ps.info()["live"] == 0 and ps.info()["ok"] == 0
                ps.close()
        finally:
            e.close()
    assert runs[0] == runs[1] == runs[2]


def test_detector_toggled_between_batches_on_one_table(eng, MAX):
    """Batches through the kernel with the detector inside alternate with plain flow batches (ppe_portscan_set able 0 / 1)
    on one table, small and large."""
    _, par = tm.generated()
    rig = gen_rig(eng, par)
    rng = np.random.default_rng(23)
    try:
        for k, (n, able) in enumerate(((300, 1), (300, 0), (MAX, 1), (3000, 0), (64, 1), (64, 0), (MAX, 1))):
            rig.able(able)
            rig.clock(10_000 + 600 * k, 1000 + k)
            hdr, lens = fpm.gen_batch(rng, n)
            rig.step(hdr, lens, outs=LAYOUTS[k % 4], what=f"n={n} able={able}")
    finally:
        rig.close()


def test_three_hundred_batches_back_to_back(eng):
    """300 batches enqueued with no synchronisation between them, then every output and both tables."""
    _, par = tm.generated()
    rig = gen_rig(eng, par)
    rng = np.random.default_rng(29)
    try:
        rig.clock(10_000, 1000)
        batches = [fpm.gen_batch(rng, int(rng.integers(1, 201))) for _ in range(300)]
        queued = [rig.enqueue(h, ln) for h, ln in batches]
        torch.cuda.synchronize()
        assert eng.flow_launch_info() == (2, 1)
        for k, ((h, ln), (out, _, cfg)) in enumerate(zip(batches, queued)):
            rig.check(out, h, ln, None, cfg, f"batch {k}")
        rig.same()
    finally:
        rig.close()


def test_attachment_points_and_refusals(eng, MAX):
    rules = tm.kat_rules()
    rig = Rig(eng, rules, attach=False)
    other = Engine(0)
    try:
        ps, lib = rig.ps, eng.lib
        hdr, lens = tm.stack([udp_packet()])
        th, tl, _ = to_dev(hdr, lens)

        def run():
            out = alloc(1, PLAIN)
            eng.classify_flow_torch(th, tl, out, cfg=eng.cfg(0, 1, 5))
            torch.cuda.synchronize()
            return out
        # a table sits on at most one of the two points
        ps.attach()
        assert lib.ppe_flow_portscan_attach(eng.ctx, ps.h) == abi.PPE_EINVAL
        with pytest.raises(PPEError, match="-95"):  # (stateless attachment: the flow path refuses, as before)
            run()
        ps.detach()
        ps.attach_flow()
        assert lib.ppe_portscan_attach(eng.ctx, ps.h) == abi.PPE_EINVAL
        assert lib.ppe_flow_portscan_attach(other.ctx, ps.h) == abi.PPE_EINVAL  # a table of another context
        run()
        assert eng.flow_launch_info() == (2, 1)
        # the stateless calls do not see a flow-attached table
        out = alloc(1, PLAIN)
        eng.classify_torch(th, tl, out, cfg=eng.cfg(0, 1, 5))
        torch.cuda.synchronize()
        assert ps.info()["ok"] == 1
        # monitors flow-attached at the same time, and stream tracking: refused before anything is touched
        atk = eng.attack(attach="flow")
        with pytest.raises(PPEError, match="-95"):
            run()
        atk.close()
        eng.stream_tcp(1, 0, 0)
        with pytest.raises(PPEError, match="-95"):
            run()
        eng.stream_tcp(0, 0, 0)
        assert ps.info()["ok"] == 1
        # the host call's list outputs stay refused; a batch above the port-scan table's max_batch is PPE_EINVAL
        small = eng.portscan(attach=False, max_batch=64)
        ps.detach_flow()
        small.attach_flow()
        h2, l2 = tm.stack([udp_packet()] * 65)
        t2, tl2, _ = to_dev(h2, l2)
        with pytest.raises(PPEError, match="-22"):
            eng.classify_flow_torch(t2, tl2, alloc(65, PLAIN), cfg=eng.cfg(0, 1, 5))
        small.close()  # ppe_portscan_destroy detaches from whichever point holds the table
        run()
        assert eng.flow_launch_info() == (1, 1) and getattr(eng, "portscan_flow_attached", None) is None
        # the steered multi-GPU flow path refuses a flow-attached table before any collective (a source's chain would
        # span ranks); detached, or destroyed, it runs (here: one rank, the exchanges handing its own rows back)
        from ppe.dist import DeviceSteerOps, steered_classify_flow

        class OneRank:
            @staticmethod
            def all_to_all_single(out, inp, **kw):
                out.copy_(inp)
        ops, cfg = DeviceSteerOps(eng), eng.cfg(0, 1, 5)
        ps.attach_flow()
        before = ps.info()
        with pytest.raises(PPEError, match="-95.*ppe_flow_portscan_attach"):
            steered_classify_flow(ops, None, th, tl, cfg, 1, 0)
        assert ps.info() == before
        ps.detach_flow()
        assert steered_classify_flow(ops, OneRank, th, tl, cfg, 1, 0)["verdict"].numel() == 1
        again = eng.portscan(attach="flow")
        with pytest.raises(PPEError, match="-95"):
            steered_classify_flow(ops, None, th, tl, cfg, 1, 0)
        again.close()
        assert steered_classify_flow(ops, OneRank, th, tl, cfg, 1, 0)["verdict"].numel() == 1
    finally:
        other.close()
        rig.close()
