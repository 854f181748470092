"""The port-scan pre-pass for small batches: one launch of one workgroup (ps_fused_kernel, n <= 2,048) against the
staged launches against the tests' serial model (tests/portscan_model.py).

Two tables with one configuration on two contexts with the same rules, one of them created under PPE_PS_FUSED=0.  After
every batch the verdict, ACL hit, flow hash and tuple, ppe_counters_t and the stream counters, the ppe_portscan_info
counts and the whole ppe_portscan_dump are equal between the two and equal to the model; 64 guard entries behind every
output stay untouched; ppe_portscan_prepass_info names the path each table took.  Integer work: no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import test_gpu_attack as ga  # noqa: E402  (its guarded output buffers and the rig with the monitors attached)
import test_gpu_portscan as gp  # noqa: E402  (its rig: engine + model + oracle)
from portscan_model import DETECTED, HOLD, NOMEM, OK  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402

NOW, R, S0, DEV = gp.NOW, gp.R, gp.S0, gp.DEV
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    yield e
    for x in e:
        x.close()


@pytest.fixture(autouse=True)
def clean_afterwards(request):
    yield
    if "engines" in request.fixturenames:
        for e in request.getfixturevalue("engines"):
            if getattr(e, "attack_attached", None) is not None:
                e.attack_attached.close()
            if getattr(e, "portscan_attached", None) is not None:
                e.portscan_attached.close()
            e.stream_tcp(0, 0, 0)


def staged(make):
    """make() with PPE_PS_FUSED=0 in the environment: ppe_portscan_create reads it, the table keeps it."""
    assert "PPE_PS_FUSED" not in os.environ
    os.environ["PPE_PS_FUSED"] = "0"
    try:
        return make()
    finally:
        del os.environ["PPE_PS_FUSED"]


class GRig(gp.Rig):
    """tests/test_gpu_portscan.py's rig with 64 guard entries behind every output."""

    def classify(self, hdr, lens, outs, ts=None):
        n = len(lens)
        th, tl, _ = ga.to_dev(hdr, lens)
        tt = torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to(DEV) if ts is not None else None
        out = ga.alloc(n, outs)
        self.eng.classify_torch(th, tl, out, cfg=self.eng.cfg(0, self.syn_check, NOW), ts=tt)
        torch.cuda.synchronize()
        return ga.collect(out, n)     # (asserts the guard entries)


def check_paths(fused_ps, staged_ps, n):
    kind, launches = fused_ps.prepass_info()
    assert (kind, launches) == (1, 1) if n <= 2048 else (kind == 0 and launches >= 10), (n, kind, launches)
    kind, launches = staged_ps.prepass_info()
    assert kind == 0 and launches >= 10, (n, kind, launches)


def same_tables(a, b):
    ia, ib = a.info(), b.info()
    assert {k: ia[k] for k in gp.INFO_KEYS} == {k: ib[k] for k in gp.INFO_KEYS}
    assert ia["slots"] == ib["slots"] and ia["rebuilds"] == ib["rebuilds"]
    assert {tuple(int(x) for x in e) for e in a.dump()} == {tuple(int(x) for x in e) for e in b.dump()}


class Pair:
    def __init__(self, engines, rules, **kw):
        self.f = GRig(engines[0], rules, **kw)
        self.s = staged(lambda: GRig(engines[1], rules, **kw))
        assert self.f.ps.prepass_info() == (0, 0)

    def clock(self, cycles, seconds):
        self.f.clock(cycles, seconds)
        self.s.clock(cycles, seconds)

    def set(self, **kw):
        for r in (self.f, self.s):
            r.ps.set(**kw)
            for k, v in kw.items():
                setattr(r.m, k, v)

    def step(self, hdr, lens, outs=gp.PLAIN, ts=None):
        ref = self.f.reference(hdr, lens, ts)
        gf, exp = self.f.step(hdr, lens, outs, ts, ref)     # fused == model: outputs, counters, info, dump
        gs, _ = self.s.step(hdr, lens, outs, ts, ref)       # staged == model
        for k in gf:
            assert np.array_equal(gf[k], gs[k]), k
        assert self.f.eng.counters() == self.s.eng.counters()
        assert self.f.eng.stream_counters() == self.s.eng.stream_counters()
        same_tables(self.f.ps, self.s.ps)
        check_paths(self.f.ps, self.s.ps, len(lens))
        return gf, exp

    def close(self):
        self.f.close()
        self.s.close()


def crowd(n, seed):
    """n packets of 40 sources (more than the 24 records), ports from a few values with zeros, interleaved."""
    rng = np.random.default_rng(seed)
    sip = (S0 + rng.integers(0, 40, n)).astype(np.uint32)
    dport = rng.choice(np.array([0, 22, 22, 23, 80, 1000, 2000], np.uint32), n)
    return sip, dport


@pytest.mark.parametrize("n", SIZES)
def test_sizes(engines, n):
    """Every size at which a phase of the one-workgroup kernel changes shape: one lane, a ragged tile, one and two keys
    per thread, the full sort block, and the first staged size.  Two batches: creation with NOMEM, then after the roll
    detections and holds (except at the sizes too small to record three changes)."""
    pair = Pair(engines, gp.port_rules(), exception_freq=3, capacity=24)
    sip, dport = crowd(n, n)
    for k, outs in enumerate((gp.SEP, gp.PART8)):
        pair.clock(50_000 + k * (R + 1), NOW + k)
        _, exp = pair.step(*gp.frames(sip, dport), outs=outs)
    if n >= 1023:
        seen = set(exp["results"].tolist())
        assert {OK, NOMEM, DETECTED, HOLD} <= seen
    pair.close()


def test_known_answers_across_batches(engines):
    """tests/test_portscan.py's known-answer sequence, one to four packets per batch: first create and counting, the
    roll, exactly rate / 2 rate, a clock that goes back, detection, hold and release by timestamp, port 0."""
    script = [(5000, 100, [80]), (5400, 100, [80, 81, 81, 82]), (6401, 101, [82]), (6401, 101, [83, 84, 85]),
              (7402, 102, [85]), (7500, 102, [85, 86, 87]), (7600, 102, [1, 2]), (8402, 103, [0, 0, 9]),
              (8402 + R, 104, [10]), (8402 + 3 * R, 106, [11, 12]), (4000, 106, [13]), (4500, 106, [0]),
              (4600, 106, [14, 15, 16, 17]), (5700, 107, [17]), (5800, 107, [18, 19])]
    pair = Pair(engines, gp.port_rules(), hold_seconds=2)
    seen = set()
    for cyc, sec, ports in script:
        pair.clock(cyc, NOW + sec)
        ts = np.full(len(ports), NOW + sec, np.uint64)
        _, exp = pair.step(*gp.frames([S0] * len(ports), ports), ts=ts)
        seen |= set(exp["results"].tolist())
    assert seen == {OK, DETECTED, HOLD}
    pair.close()
    pair = Pair(engines, gp.port_rules(), hold_seconds=0)      # every change detects, nothing is held
    for cyc, ports in ((5000, [80, 81, 82, 83]), (6500, [83]), (6600, [84, 85, 85, 86])):
        pair.clock(cyc, NOW)
        _, exp = pair.step(*gp.frames([S0] * len(ports), ports))
    assert exp["results"].tolist() == [DETECTED, DETECTED, OK, DETECTED]
    pair.close()


def test_one_source_owns_the_sort_block(engines):
    """One source, 2,048 packets: a window that reaches exception_freq; after the roll a new port per packet: the walker
    inside the workgroup detects at the first change, then HOLD; a third batch is held from its first packet, and a
    timestamp past the hold releases it mid-batch."""
    n = 2048
    rng = np.random.default_rng(11)
    dport = rng.integers(1, 50, n).astype(np.uint32)
    sip = np.full(n, S0, np.uint32)
    pair = Pair(engines, gp.port_rules(), exception_freq=50, hold_seconds=5)
    _, exp = pair.step(*gp.frames(sip, dport))
    assert (exp["results"] == OK).all()
    pair.clock(50_000 + R + 1, NOW + 1)
    d2 = (3000 + np.arange(n)).astype(np.uint32)
    d2[0] = dport[-1]                                       # the first change is packet 1
    _, exp = pair.step(*gp.frames(sip, d2))
    assert exp["results"][0] == OK and exp["results"][1] == DETECTED and (exp["results"][2:] == HOLD).all()
    pair.clock(50_000 + R + 900, NOW + 2)
    ts = np.full(n, NOW + 2, np.uint64)
    ts[1500:] = NOW + 6                                     # hold = NOW + 1 + 5: released at packet 1,500
    _, exp = pair.step(*gp.frames(sip, d2), ts=ts)
    assert (exp["results"][:1500] == HOLD).all() and (exp["results"][1500:] != HOLD).any()
    pair.close()


def test_grant_order(engines):
    """2,048 distinct sources against 3 free records: the first three by first appearance get them, in a permuted
    batch too; then one record is free again after aging."""
    n = 2048
    rng = np.random.default_rng(3)
    sip = (S0 + rng.permutation(n)).astype(np.uint32)
    dport = rng.integers(20, 25, n).astype(np.uint32)
    pair = Pair(engines, gp.port_rules(), capacity=3, exception_freq=1000)
    _, exp = pair.step(*gp.frames(sip, dport), outs=gp.PART)
    assert (exp["results"] == NOMEM).sum() == n - 3 and (exp["results"][:3] == OK).all()
    _, exp = pair.step(*gp.frames(sip[::-1].copy(), dport), outs=gp.PART)
    assert (exp["results"] == NOMEM).sum() == n - 3 and (exp["results"][-3:] == OK).all()
    now = 50_000 + 20 * R + 1
    for r in (pair.f, pair.s):
        assert r.ps.age(now) == r.m.timeout(now) == 3
    pair.clock(now + 1, NOW + 21)
    _, exp = pair.step(*gp.frames(sip[5:70].copy(), dport[5:70]), outs=gp.PART)   # 65 packets: a ragged second tile
    assert (exp["results"][:3] == OK).all() and (exp["results"][3:] == NOMEM).all()
    pair.close()


@pytest.mark.parametrize("syn_check", [1, 0])
def test_eligibility(engines, syn_check):
    """Malformed frames, fragments, VLAN, UDP, TCP with and without SYN: only what reaches the ACL reaches the detector,
    with syn_check on and off; 1, 65, 130 and 450 packets (ragged last tiles)."""
    hdr, lens = gp.eligibility_batch()
    pair = Pair(engines, synth.make_rules(256, seed=256), syn_check=syn_check, exception_freq=0, capacity=40)
    for lo, n in ((0, 1), (1, 65), (66, 130), (0, 450)):
        _, exp = pair.step(hdr[lo:lo + n], lens[lo:lo + n], outs=gp.SEP)
    st = exp["verdict"] & 0xFF
    assert (exp["results"] < 0).sum() > 20 and (st == ST["PORTSCAN_DROP"]).sum() > 0
    assert ((st == ST["FLOW_TCP_NO_SYN_FIRST"]).sum() > 0) == (syn_check == 1)
    pair.close()


def test_action_forward(engines):
    """action = 1: nothing is dropped, detection and state still run, on both paths."""
    sip, dport = gp.interleaved(64)
    pair = Pair(engines, gp.port_rules(), action=1, exception_freq=0)
    _, exp = pair.step(*gp.frames(sip, dport), outs=gp.SEP)
    assert (exp["results"] == DETECTED).any() and (exp["results"] == HOLD).any() and pair.f.ps.info()["drop"] == 0
    assert not ((exp["verdict"] & 0xFF) == ST["PORTSCAN_DROP"]).any()
    pair.close()


def test_with_attack_monitors(engines):
    """The ATK instantiation: with the monitors attached on the stateless point a land- or flood-dropped SYN never
    reaches the detector, in the one-launch kernel as in the staged find kernel."""
    hdr, lens = ga.scanner(120)
    kw = dict(pd={0: dict(land=1, drop_pack=1)}, td={0: dict(flood_syn=1, syn_speed=50, syn_count=1 << 30, drop_pack=1)},
              hold=3, portscan=dict(exception_freq=0, capacity=64))
    rigs = (ga.Rig(engines[0], **kw), staged(lambda: ga.Rig(engines[1], **kw)))
    for what in ("land only", "flood"):
        exps = [r.step(hdr, lens, what=what)[1] for r in rigs]      # each == the composed model
        st = exps[0]["verdict"] & 0xFF
        assert np.array_equal(exps[0]["verdict"], exps[1]["verdict"]) and (st == ga.LAND).sum() == 40
        same_tables(rigs[0].ps, rigs[1].ps)
        check_paths(rigs[0].ps, rigs[1].ps, len(lens))
        if what == "land only":
            assert (st == ST["PORTSCAN_DROP"]).any()
            for r in rigs:
                r.tick(NOW + 1)
        else:
            assert (st == ga.SYNF).sum() == 81
    for r in rigs:
        r.close()


def test_ring_call_mixes_both_paths(engines):
    """ppe_classify_batches over five batches of 2,048, 1, 4,096, 65 and 2,049 packets (one-launch, one-launch, staged,
    one-launch, staged pre-passes in one call) equals five single calls on the staged table, and the model."""
    sizes = (2048, 1, 4096, 65, 2049)
    pair = Pair(engines, gp.port_rules(), exception_freq=3, capacity=24)
    eng = pair.f.eng
    old = eng.tuning()
    eng.tuning(batches_per_launch=0)
    try:
        pair.step(*gp.frames(*crowd(512, 1)))                   # a window of changes, then the roll
        pair.clock(50_000 + R + 1, NOW + 1)
        keep, exps = [], []
        for j, m in enumerate(sizes):
            hdr, lens = gp.frames(*crowd(m, 100 + j))
            ref = pair.f.reference(hdr, lens)
            exps.append(pair.f.m.expected(ref, hdr, now_seconds=NOW))
            pair.s.step(hdr, lens, ref=ref)                     # the single call on the staged table
            th, tl, _ = ga.to_dev(hdr, lens)
            out = ga.alloc(m, ("verdict", "flow_hash", "acl_hit"))
            keep.append((abi.Batch(th.data_ptr(), tl.data_ptr(), None, m, 64),
                         abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(),
                                    None, None, None, None), th, tl, out))
        nb = len(sizes)
        ins, outs = (abi.Batch * nb)(*(k[0] for k in keep)), (abi.Result * nb)(*(k[1] for k in keep))
        cfg = eng.cfg(0, 1, NOW)
        s = torch.cuda.current_stream(DEV)
        eng.clear_counters()
        assert eng.lib.ppe_classify_batches(eng.ctx, ins, outs, nb, C.byref(cfg), C.c_void_p(s.cuda_stream)) == 0
        torch.cuda.synchronize()
        for k, e, m in zip(keep, exps, sizes):
            got = ga.collect(k[4], m)
            for name in ("verdict", "flow_hash", "acl_hit"):
                assert np.array_equal(got[name], e[name]), (m, name)
        assert eng.counters() == {k: sum(e["counters"][k] for e in exps) for k in abi.COUNTERS}
        pair.f.check_table()
        same_tables(pair.f.ps, pair.s.ps)
        check_paths(pair.f.ps, pair.s.ps, sizes[-1])
        assert any((e["results"] == DETECTED).any() for e in exps) and (exps[-1]["results"] == HOLD).any()
    finally:
        eng.tuning(**old)
        pair.close()
