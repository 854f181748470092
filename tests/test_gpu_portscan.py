"""The port-scan detector on the stateless classify path (ppe_portscan_*) on the GPU, exact against the oracle's result
rewritten by the tests' serial model (tests/portscan_model.py): verdict word, ACL hit, flow hash, tuple, ppe_counters_t,
the stream counters, the ppe_portscan_info counts and the dumped records (as a set), after every batch.

Integer work: no tolerance anywhere.  Known answers use exception_freq = 3 and 1,000 cycles per second."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
import decode_corpus as dc  # noqa: E402
import stream_model as sm  # noqa: E402
from pktbuild import ip_frag, tcp_packet, udp_packet  # noqa: E402
from portscan_model import DETECTED, HOLD, NOMEM, OK, PortScanModel  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402

NOW = 1_700_000_000
DEV = torch.device("cuda:0")
R = 1000
S0 = 0x0A000001
SEP = ("verdict", "flow_hash", "acl_hit", "fw_idx", "drop_idx", "tile_cnt", "tuple")
PART = ("verdict", "flow_hash", "acl_hit", "part_idx")
PART8 = ("verdict", "flow_hash", "acl_hit", "part8")
PACKED = ("packed", "part8")
PLAIN = ("verdict", "flow_hash", "acl_hit", "tuple")
INFO_KEYS = ("live", "new_pcb", "del_pcb", "ok", "nomem", "detected", "hold", "drop")


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def clean_afterwards(request):
    yield
    if "eng" in request.fixturenames:
        e = request.getfixturevalue("eng")
        if getattr(e, "portscan_attached", None) is not None:
            e.portscan_attached.close()
        e.stream_tcp(0, 0, 0)


def port_rules():
    """dport 1000-1999 forwards (rule 0), 2000-2999 drops (rule 1), any address and protocol; default FW."""
    r = np.zeros(2, abi.RULE_DTYPE)
    r["sport_end"] = 65535
    r["protocol_end"] = 255
    r["dport_start"], r["dport_end"] = (1000, 2000), (1999, 2999)
    r["action"] = (abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP)
    return r


_UDP = np.frombuffer(udp_packet(), np.uint8)
_TCP = np.frombuffer(tcp_packet(payload=b"\0" * 10), np.uint8)


def frames(sip, dport, stride=64, tcp_flags=None):
    """64-B UDP frames (or TCP with the given flags byte) from arrays of source addresses and destination ports."""
    sip, dport = np.asarray(sip, np.uint32), np.asarray(dport, np.uint32)
    n = len(sip)
    hdr = np.zeros((n, stride), np.uint8)
    hdr[:, :64] = _UDP if tcp_flags is None else _TCP
    for k in range(4):
        hdr[:, 26 + k] = (sip >> (24 - 8 * k)) & 0xFF
    hdr[:, 36], hdr[:, 37] = dport >> 8, dport & 0xFF
    if tcp_flags is not None:
        hdr[:, 47] = tcp_flags
    return hdr, np.full(n, 64, np.uint32)


class Rig:
    """An engine with a table attached, the model beside it and the oracle for the rule set: step() runs one batch
    through both and compares everything."""

    def __init__(self, eng, rules, default_action=abi.ACL_RULE_ACTION_FW, stream=None, syn_check=1, attach=True, **cfg):
        d = dict(exception_freq=3, hold_seconds=600, capacity=64, max_batch=4096, cycles_per_second=R)
        d.update(cfg)
        self.eng, self.syn_check, self.stream = eng, syn_check, stream
        eng.commit(rules, default_action=default_action)
        eng.stream_tcp(*(stream or (0, 0, 0)))
        self.ps = eng.portscan(attach=attach, **d)
        md = {k: v for k, v in d.items() if k != "max_batch"}
        self.m = PortScanModel(**md)
        self.o = pyoracle.Oracle(rules, default_action=default_action)
        self.clock(50_000, NOW)

    def clock(self, cycles, seconds):
        self.ps.clock(cycles, seconds)
        self.m.clock(cycles, seconds)

    def close(self):
        self.ps.close()

    def classify(self, hdr, lens, outs, ts=None):
        n = len(lens)
        th = torch.from_numpy(np.ascontiguousarray(hdr)).to(DEV)
        tl = torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32)).to(DEV)
        tt = torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to(DEV) if ts is not None else None
        shapes = {"tile_cnt": ((n + 63) // 64,), "tuple": (n, 4)}
        out = {k: torch.full(shapes.get(k, (n,)), -7, dtype=torch.int32, device=DEV) for k in outs
               if k not in ("part8", "packed")}
        if "part8" in outs:
            out["part8"] = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=DEV)
        if "packed" in outs:
            out["packed"] = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        self.eng.classify_torch(th, tl, out, cfg=self.eng.cfg(0, self.syn_check, NOW), ts=tt)
        torch.cuda.synchronize()
        res = {}
        for k, v in out.items():
            a = v.cpu().numpy()
            res[k] = a if k in ("acl_hit", "part8") else a.view(np.uint64) if k == "packed" else a.view(np.uint32)
        if "packed" in res:
            res.update(abi.unpack(res["packed"]))
        return res

    def reference(self, hdr, lens, ts=None):
        ref = self.o.classify_batch(hdr, lens, ts=ts, cfg=self.o.cfg(0, self.syn_check, NOW))
        assert (ref["reach"] <= hdr.shape[1]).all()   # nothing is a WINDOW_PUNT at this stride
        return ref

    def step(self, hdr, lens, outs=PLAIN, ts=None, ref=None):
        n = len(lens)
        self.eng.clear_counters()
        self.eng.clear_stream_counters()
        if ref is None:
            ref = self.reference(hdr, lens, ts)
        sc = dict(zip(("track", "midstream", "async_oneside"), self.stream or (0, 0, 0)))
        exp = self.last_exp = self.m.expected(ref, hdr, ts=ts, now_seconds=NOW, stream=sc)
        got = self.classify(hdr, lens, outs, ts)
        for k in ("verdict", "flow_hash", "acl_hit") + (("tuple",) if "tuple" in got else ()):
            assert np.array_equal(got[k], exp[k]), (k, np.flatnonzero((got[k] != exp[k]).reshape(n, -1).any(axis=1))[:8],
                                                    got[k][:8], exp[k][:8])
        if "packed" in got:
            assert np.array_equal(got["packed"], sm.packed(exp["verdict"], exp["flow_hash"], exp["acl_hit"]))
        want = sm.lists(exp["verdict"])
        for k in ("fw_idx", "drop_idx", "tile_cnt", "part_idx"):
            if k in got:
                assert np.array_equal(got[k], want[k]), k
        if "part8" in got:
            assert np.array_equal(got["part8"][:n], want["part8"]) and (got["part8"][n:] == 0xEE).all()
        assert self.eng.counters() == exp["counters"]
        assert self.eng.stream_counters() == exp["stream"]
        self.check_table()
        return got, exp

    def check_table(self):
        info = self.ps.info()
        assert {k: info[k] for k in INFO_KEYS} == {k: self.m.info()[k] for k in INFO_KEYS}
        d = self.ps.dump()
        recs = {tuple(int(x) for x in e) for e in d}
        assert recs == self.m.records()


def test_known_answers_across_batches(eng):
    """One source, one to four packets per batch, the clock moved between batches: the CPU known answers
    (tests/test_portscan.py) on the GPU: first create, counting, the roll, exactly rate / 2 rate, a clock that goes
    back, detection, HOLD until the timestamp reaches the hold, hold_seconds 0, port 0, and the frozen scenario."""
    script = [(5000, 100, [80]), (5400, 100, [80, 81, 81, 82]), (6401, 101, [82]), (6401, 101, [83, 84, 85]),
              (7402, 102, [85]), (7500, 102, [85, 86, 87]), (7600, 102, [1, 2]), (8402, 103, [0, 0, 9]),
              (8402 + R, 104, [10]), (8402 + 3 * R, 106, [11, 12]), (4000, 106, [13]), (4500, 106, [0]),
              (4600, 106, [14, 15, 16, 17]), (5700, 107, [17]), (5800, 107, [18, 19])]
    rig = Rig(eng, port_rules(), hold_seconds=2)
    seen = set()
    for cyc, sec, ports in script:
        rig.clock(cyc, NOW + sec)
        hdr, lens = frames([S0] * len(ports), ports)
        ts = np.full(len(ports), NOW + sec, np.uint64)
        _, exp = rig.step(hdr, lens, ts=ts)
        seen |= set(exp["results"].tolist())
    assert seen == {OK, DETECTED, HOLD}
    rig.close()
    # hold_seconds = 0: every change detects, nothing is held
    rig = Rig(eng, port_rules(), hold_seconds=0)
    for cyc, ports in ((5000, [80, 81, 82, 83]), (6500, [83]), (6600, [84, 85, 85, 86])):
        rig.clock(cyc, NOW)
        _, exp = rig.step(*frames([S0] * len(ports), ports))
    assert exp["results"].tolist() == [DETECTED, DETECTED, OK, DETECTED]
    rig.close()
    # the frozen scenario (tests/golden/portscan_v1.npz): per-packet results as recorded, aging after batch 5
    g = np.load(Path(__file__).resolve().parent / "golden" / "portscan_v1.npz")
    rig = Rig(eng, port_rules(), exception_freq=3, hold_seconds=5, capacity=6)
    for b in range(8):
        rig.clock(int(g[f"clock{b}"][0]), int(g[f"clock{b}"][1]))
        hdr, lens = frames(g[f"sip{b}"], g[f"dport{b}"])
        _, exp = rig.step(hdr, lens, ts=g[f"ts{b}"])
        assert np.array_equal(exp["results"], g[f"res{b}"].astype(np.int64))
        if b == 5:
            now = int(g["clock5"][0]) + 25_000
            assert rig.ps.age(now) == rig.m.timeout(now) == int(g["freed5"][0])
            rig.check_table()
    rig.close()


def interleaved(stride):
    rng = np.random.default_rng(5)
    seqs = [rng.choice(np.array(p, np.uint32), 256) for p in
            ([80], [80, 81], [0, 22, 22, 23], [1000, 1001, 1002, 2000, 0], np.arange(3000, 3040))]
    src = rng.integers(0, 5, 256)
    dport = np.array([seqs[s][i] for i, s in enumerate(src)], np.uint32)
    return (S0 + src).astype(np.uint32), dport


@pytest.mark.parametrize("stride", [64, 144])
def test_order_within_a_batch(eng, stride):
    """256 packets, five sources interleaved, port sequences with repeats and zeros; then the same packets reversed
    from the same state: the model's answer differs, and the engine follows it."""
    sip, dport = interleaved(stride)
    got = []
    for rev in (False, True):
        rig = Rig(eng, port_rules(), exception_freq=3)
        rig.step(*frames(sip[:64], dport[:64], stride))     # a window to roll: exceptions recorded
        rig.clock(50_000 + R + 1, NOW + 1)
        a, b = (sip[::-1], dport[::-1]) if rev else (sip, dport)
        g, exp = rig.step(*frames(a, b, stride))
        got.append((g["verdict"][::-1] if rev else g["verdict"], rig.m.records()))
        assert (exp["results"] == DETECTED).any() and (exp["results"] == HOLD).any()
        rig.close()
    assert not np.array_equal(got[0][0], got[1][0]) and got[0][1] != got[1][1]


def test_group_sizes(eng):
    """Sources with 1, 63, 64, 65 and 1,025 packets (and many single-packet ones) in one 4,096-packet batch, twice
    (the second time with detection possible for the sources that changed ports enough)."""
    rng = np.random.default_rng(9)
    sizes = [1, 63, 64, 65, 1025]
    sip = np.concatenate([np.full(s, S0 + i, np.uint32) for i, s in enumerate(sizes)] +
                         [S0 + 100 + np.arange(4096 - sum(sizes), dtype=np.uint32) % 1500])
    dport = rng.integers(0, 6, 4096).astype(np.uint32) * 7
    dport[:sum(sizes)] += 7                   # (port 0 would keep re-arming the five sources' windows)
    perm = rng.permutation(4096)
    rig = Rig(eng, port_rules(), exception_freq=3, capacity=2000)
    rig.step(*frames(sip[perm], dport[perm]))
    rig.clock(50_000 + R + 5, NOW + 1)
    _, exp = rig.step(*frames(sip[perm], dport[perm]))
    assert (exp["results"] == DETECTED).sum() >= 4 and (exp["results"] == HOLD).sum() > 1000
    rig.close()


def test_one_source_owns_the_batch(eng):
    """One source, 65,536 packets, three times: no detection possible; detection at member 1,000 then HOLD; held."""
    n = 65536
    rng = np.random.default_rng(11)
    dport = rng.integers(1, 50, n).astype(np.uint32)
    rig = Rig(eng, port_rules(), exception_freq=50, max_batch=n)
    hdr, lens = frames(np.full(n, S0, np.uint32), dport)
    ref = rig.reference(hdr, lens)
    _, exp = rig.step(hdr, lens, ref=ref)
    assert (exp["results"] == OK).all()
    rig.clock(50_000 + R + 1, NOW + 1)        # the roll: last_exception = tens of thousands
    d2 = dport.copy()
    d2[:1001] = dport[n - 1]                  # no change before member 1,000
    d2[1000] = 7777
    hdr, lens = frames(np.full(n, S0, np.uint32), d2)
    _, exp = rig.step(hdr, lens)
    assert exp["results"][999] == OK and exp["results"][1000] == DETECTED and (exp["results"][1001:] == HOLD).all()
    rig.clock(50_000 + R + 900, NOW + 2)
    _, exp = rig.step(hdr, lens)
    assert (exp["results"] == HOLD).all()
    rig.close()


def eligibility_batch():
    sw = synth.make_tcp_flag_sweep(np.zeros(0, abi.RULE_DTYPE), stride=128)
    hdr, lens = sw["hdr"][:450].copy(), sw["len"][:450].copy()
    fr = [ip_frag(17, S0, 0x0A000002, 7, 0, 1, b"\0" * 24), ip_frag(6, S0 + 1, 0x0A000002, 8, 24, 0, b"\0" * 16)]
    for i, f in enumerate(fr):
        hdr[100 + i] = 0
        hdr[100 + i, :len(f)] = np.frombuffer(f, np.uint8)
        lens[100 + i] = len(f)
    return hdr, lens


@pytest.mark.parametrize("syn_check", [1, 0])
def test_eligibility(eng, syn_check):
    """Malformed frames, fragments, VLAN, UDP, TCP with and without SYN, the TCP header behind IPv4 options: only what
    reaches the ACL reaches the detector; n = 1, 65, 130 (tail lanes) and the whole mix."""
    hdr, lens = eligibility_batch()
    rig = Rig(eng, synth.make_rules(256, seed=256), syn_check=syn_check, exception_freq=0, capacity=40)
    for lo, n in ((0, 1), (1, 65), (66, 130), (0, 450)):
        _, exp = rig.step(hdr[lo:lo + n], lens[lo:lo + n], outs=SEP)
    st = exp["verdict"] & 0xFF
    assert (exp["results"] < 0).sum() > 20 and (st == ST["FRAG"]).sum() >= 2 and (st == ST["PORTSCAN_DROP"]).sum() > 0
    assert ((st == ST["FLOW_TCP_NO_SYN_FIRST"]).sum() > 0) == (syn_check == 1)
    assert (exp["results"][st == ST["FLOW_TCP_NO_SYN_FIRST"]] < 0).all()
    rig.close()


def test_capacity_and_aging(eng):
    """Capacity 8, 12 new sources in one batch: the first eight by first appearance get records; after aging the
    same batch again."""
    rng = np.random.default_rng(3)
    sip = (S0 + rng.permutation(np.repeat(np.arange(12), 9))).astype(np.uint32)
    dport = rng.integers(20, 25, len(sip)).astype(np.uint32)
    rig = Rig(eng, port_rules(), capacity=8, exception_freq=1000)
    _, exp = rig.step(*frames(sip, dport), outs=PART)
    assert (exp["results"] == NOMEM).sum() == 36 and rig.m.info()["live"] == 8
    _, exp = rig.step(*frames(sip[::-1], dport), outs=PART)      # the refused sources stay refused
    assert (exp["results"] == NOMEM).sum() == 36
    now = 50_000 + 20 * R
    assert rig.ps.age(now) == rig.m.timeout(now) == 0            # == 20 rate stays
    assert rig.ps.age(now + 1) == rig.m.timeout(now + 1) == 8
    rig.check_table()
    rig.clock(now + 2, NOW + 21)
    _, exp = rig.step(*frames(sip[::-1], dport), outs=PART)      # another eight, by the new order
    assert (exp["results"] == NOMEM).sum() == 36 and rig.ps.info()["rebuilds"] == 2
    rig.close()


def test_action_forward(eng):
    """action = 1: results and ppe_counters_t equal a context with no table; info counts and records equal the model."""
    sip, dport = interleaved(64)
    hdr, lens = frames(sip, dport)
    rig = Rig(eng, port_rules(), action=1, exception_freq=0)
    got, exp = rig.step(hdr, lens, outs=SEP)
    cnt = eng.counters()
    assert (exp["results"] == DETECTED).any() and (exp["results"] == HOLD).any() and rig.ps.info()["drop"] == 0
    rig.close()
    eng.clear_counters()
    plain = Rig.classify(rig, hdr, lens, SEP)
    for k in SEP:
        assert np.array_equal(got[k], plain[k]), k
    assert eng.counters() == cnt


def test_no_acl_and_no_stream_counter_for_a_dropped_packet(eng):
    """Dropped packets would have hit the FW rule and the DROP rule: no ACL_* is counted for them; with StreamTcp at
    the reference's defaults a port-scan-dropped RST counts in no stream counter."""
    n = 300
    dport = np.where(np.arange(n) % 2 == 0, 1000 + np.arange(n) % 900, 2000 + np.arange(n) % 900).astype(np.uint32)
    hdr, lens = frames(np.full(n, S0, np.uint32), dport, tcp_flags=0x06)   # SYN | RST
    hdr[3::7, 47] = 0x02                                                    # some plain SYNs
    rig = Rig(eng, port_rules(), stream=(1, 0, 0), exception_freq=0)
    _, exp = rig.step(hdr[:4], lens[:4], outs=SEP)
    assert exp["stream"]["rst_but_no_session"] == 1 and exp["stream"]["rst_count"] == 1   # packet 0 only: OK
    rig.ps.set(hold_seconds=0)
    rig.m.hold_seconds = 0
    rig.clock(50_000 + 1, NOW + 700)
    _, exp = rig.step(hdr, lens, outs=SEP)
    c = exp["counters"]
    dropped = int(((exp["verdict"] & 0xFF) == ST["PORTSCAN_DROP"]).sum())
    assert dropped > 250 and c["acl_fw"] + c["acl_drop"] == n - dropped and c["flow_proc_fail"] >= dropped
    assert exp["stream"]["rst_count"] < 10
    rig.close()


TUNINGS = [dict(lds_image=0), dict(block=512), dict(pipeline=1), dict(pipeline=4), dict(pipeline=1, lds_image=0),
           dict(pipeline=4, lds_image=0), dict(pipeline=4, block=1024), dict(pipeline=3), dict(pipeline=3, lds_image=0),
           dict(pipeline=5), dict(pipeline=5, block=1024), dict(pipeline=5, lds_image=0), dict(pipeline=5, block=256)]
_mixed = {}


def mixed(rules_name, stride):
    """The StreamTcp sweep (every TCP flag combination, VLAN, ihl 6, UDP, malformed; its sources are mostly distinct,
    so a small table refuses most) with a scanner's and two quiet sources' frames spliced in."""
    if (rules_name, stride) not in _mixed:
        rules = synth.make_rules(int(rules_name), seed=int(rules_name))
        sw = synth.make_tcp_flag_sweep(rules, stride=stride, repeat=2)
        hdr, lens = sw["hdr"].copy(), sw["len"].copy()
        idx = np.arange(3, len(lens), 5)
        k = len(idx)
        own, _ = frames(S0 + (np.arange(k) % 3 == 0).astype(np.uint32), 1000 + np.arange(k) // 2, stride,
                        tcp_flags=0x02)
        own[1::4, 47] = 0x06
        hdr[idx], lens[idx] = own, 64
        o = pyoracle.Oracle(rules, default_action=abi.ACL_RULE_ACTION_FW)
        ref = o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW), nthreads=4)
        if stride >= 128:
            assert (ref["reach"] <= stride).all()
        _mixed[(rules_name, stride)] = (rules, hdr, lens, ref)
    return _mixed[(rules_name, stride)]


@pytest.mark.parametrize("tune", TUNINGS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_kernel_variants_and_layouts(eng, tune):
    """Every output layout (SoA with lists and tile counts, partition, part8, packed) under the launch variants
    tests/test_gpu_stream_tcp.py sweeps (pipelines 1, 3, 4, 5; LDS, global and split images), 256 and 4,096 rules, with
    and without StreamTcp: the PSC kernels and the PSC + STM kernels."""
    for rules_name in ("256", "4096"):
        rules, hdr, lens, ref = mixed(rules_name, 128)
        for stream in (None, (1, 0, 0)):
            rig = Rig(eng, rules, stream=stream, exception_freq=3, capacity=48)
            old = eng.tuning()
            try:
                eng.tuning(**tune)
                for k, outs in enumerate((SEP, PART, PART8, PACKED)):
                    rig.clock(50_000 + k * (R + 1), NOW + k)
                    got, exp = rig.step(hdr, lens, outs=outs, ref=ref)
            finally:
                eng.tuning(**old)
                rig.close()
            st = exp["verdict"] & 0xFF
            assert (st == ST["PORTSCAN_DROP"]).sum() > 300 and (exp["results"] == NOMEM).any()
            if stream:
                assert (st == ST["STREAM_RST_NO_SESSION"]).sum() > 0


def test_batches_in_one_ring_launch(eng):
    """ppe_classify_batches with three batches (and with 34: the descriptor ring) in one launch equals the model
    running the batches one after the other, which is what three ppe_classify calls give."""
    sip, dport = interleaved(64)
    for nb in (3, 34):
        rig = Rig(eng, port_rules(), exception_freq=3)
        eng.tuning(batches_per_launch=0)
        rig.step(*frames(sip, dport))             # a window of changes, then the roll: detections in the launch
        rig.clock(50_000 + R + 1, NOW + 1)
        keep, exps = [], []
        for j in range(nb):
            m = 256 - 3 * j
            hdr, lens = frames(np.roll(sip, j)[:m], np.roll(dport, 2 * j)[:m])
            exps.append(rig.m.expected(rig.reference(hdr, lens), hdr, now_seconds=NOW))
            th, tl = torch.from_numpy(hdr).to(DEV), torch.from_numpy(lens.view(np.int32)).to(DEV)
            out = {k: torch.full((m,), -7, dtype=torch.int32, device=DEV) for k in ("verdict", "flow_hash", "acl_hit")}
            keep.append((abi.Batch(th.data_ptr(), tl.data_ptr(), None, m, 64),
                         abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(),
                                    None, None, None, None), th, tl, out))
        ins, outs = (abi.Batch * nb)(*(k[0] for k in keep)), (abi.Result * nb)(*(k[1] for k in keep))
        cfg = eng.cfg(0, 1, NOW)
        s = torch.cuda.current_stream(DEV)
        eng.clear_counters()
        assert eng.lib.ppe_classify_batches(eng.ctx, ins, outs, nb, C.byref(cfg), C.c_void_p(s.cuda_stream)) == 0
        torch.cuda.synchronize()
        for k, e in zip(keep, exps):
            assert np.array_equal(k[4]["verdict"].cpu().numpy().view(np.uint32), e["verdict"])
            assert np.array_equal(k[4]["acl_hit"].cpu().numpy(), e["acl_hit"])
            assert np.array_equal(k[4]["flow_hash"].cpu().numpy().view(np.uint32), e["flow_hash"])
        total = {k: sum(e["counters"][k] for e in exps) for k in abi.COUNTERS}
        assert eng.counters() == total
        assert (exps[0]["results"] == DETECTED).any() and (exps[-1]["results"] == HOLD).any()
        rig.check_table()
        rig.close()


def test_detached_or_disabled_is_identical(eng):
    """Detached, or able = 0: outputs and counters byte-identical to a context that never had a table."""
    rules, hdr, lens, ref = mixed("256", 128)
    base_eng = Engine(0)
    try:
        base_eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
        rig0 = Rig.__new__(Rig)
        rig0.eng, rig0.syn_check = base_eng, 1
        base = rig0.classify(hdr, lens, SEP)
        base_cnt = base_eng.counters()
    finally:
        base_eng.close()
    for k in ("verdict", "flow_hash", "acl_hit", "tuple"):
        assert np.array_equal(base[k], ref[k]), k
    rig = Rig(eng, rules, exception_freq=0, capacity=8)
    rig.step(hdr, lens, outs=SEP, ref=ref)                      # attached: drops
    for how in ("able0", "detached"):
        if how == "able0":
            rig.ps.set(able=0)
        else:
            rig.ps.set(able=1)
            rig.ps.detach()
        before = rig.ps.info()
        eng.clear_counters()
        got = rig.classify(hdr, lens, SEP)
        for k in SEP:
            assert np.array_equal(got[k], base[k]), (how, k)
        assert eng.counters() == base_cnt
        after = rig.ps.info()
        assert {k: after[k] for k in INFO_KEYS} == {k: before[k] for k in INFO_KEYS}   # the table stood still
    rig.close()


def test_not_supported_calls_leave_everything_usable(eng):
    """PPE_ENOTSUP from ppe_classify_flow, ppe_classify_host and the steered path with a table attached; nothing is
    touched, and both tables work afterwards.  able / action above 1: PPE_EINVAL."""
    lib = eng.lib
    for bad in ((2, 0), (0, 2)):
        c, h = abi.PortScanCfg(bad[0], bad[1], 50, 600, 0, 0, 0, 0), C.c_void_p()
        assert lib.ppe_portscan_create(eng.ctx, C.byref(c), C.byref(h)) == abi.PPE_EINVAL and not h
    rules = synth.make_rules(256, seed=256)
    rig = Rig(eng, rules, exception_freq=3, capacity=5000)
    c = abi.PortScanCfg(1, 3, 50, 600, 0, 0, 0, 0)
    assert lib.ppe_portscan_set(rig.ps.h, C.byref(c)) == abi.PPE_EINVAL and rig.ps.info()["cfg"]["action"] == 0
    pk = synth.make_flow_packets(4096, rules, n_flows=600, seed=21, syn_frac=0.6)
    th = torch.from_numpy(pk["hdr"]).to(DEV)
    tl = torch.from_numpy(pk["len"].view(np.int32)).to(DEV)
    out = {k: torch.full((4096,), -7, dtype=torch.int32, device=DEV) for k in ("verdict", "flow_hash", "acl_hit")}
    b = abi.Batch(th.data_ptr(), tl.data_ptr(), None, 4096, 64)
    r = abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(), None, None,
                   None, None)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    cfg = eng.cfg(0, 1, NOW)
    eng.flow_create(10_000, 4096)
    o = pyoracle.Oracle(rules, default_action=abi.ACL_RULE_ACTION_FW)
    ft = pyoracle.OracleFlow(o, capacity=10_000)
    try:
        assert lib.ppe_classify_flow(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), s) == abi.PPE_ENOTSUP
        hv = np.full(256, 0xFFFFFFF9, np.uint32)
        hh, hl = pk["hdr"][:256].copy(), pk["len"][:256].copy()
        hb = abi.Batch(hh.ctypes.data, hl.ctypes.data, None, 256, 64)
        hr = abi.Result(hv.ctypes.data, None, None, None, None, None, None)
        assert lib.ppe_classify_host(eng.ctx, C.byref(hb), C.byref(hr), C.byref(cfg), 0) == abi.PPE_ENOTSUP
        from ppe.dist import DeviceSteerOps, steered_classify_flow
        with pytest.raises(PPEError, match="-95"):  # before any collective: no process group is needed to see it
            steered_classify_flow(DeviceSteerOps(eng), None, th, tl, cfg, 1, 0)
        torch.cuda.synchronize()
        assert (out["verdict"].cpu().numpy() == -7).all() and (hv == 0xFFFFFFF9).all()   # nothing ran
        assert eng.flow_info()["live"] == 0 and rig.ps.info()["live"] == 0
        rig.step(pk["hdr"], pk["len"])                          # the port-scan table works
        rig.ps.detach()
        eng.classify_flow_torch(th, tl, out, cfg=cfg)           # and so does the flow table
        torch.cuda.synchronize()
        ref = ft.classify_batch(pk["hdr"], pk["len"], cfg=o.cfg(0, 1, NOW))
        assert np.array_equal(out["verdict"].cpu().numpy().view(np.uint32), ref["verdict"])
        assert eng.flow_info()["live"] == ft.stats()["live"] > 0
        assert lib.ppe_classify_host(eng.ctx, C.byref(hb), C.byref(hr), C.byref(cfg), 0) == 0
    finally:
        eng.flow_destroy()
        rig.close()


@pytest.mark.parametrize("nrules", [256, 4096])
@pytest.mark.parametrize("stream", [None, (1, 0, 0)], ids=["plain", "stream"])
@pytest.mark.parametrize("syn_check", [1, 0])
def test_decode_edge_corpus(eng, syn_check, stream, nrules):
    """The pre-pass decodes every packet itself: its eligibility must equal "reached the ACL" on every edge of the
    decode (tests/decode_corpus.py, 128-B windows: nothing punts).  One frame, 64 frames from an odd offset, then the
    whole corpus, into a table of 40 records that every eligible packet trips (exception_freq 0)."""
    rules = synth.make_rules(nrules, seed=nrules)
    hdr, lens, _ = dc.corpus(rules)
    hdr = np.ascontiguousarray(hdr[:, :128])
    rig = Rig(eng, rules, stream=stream, syn_check=syn_check, exception_freq=0, capacity=40)
    try:
        for lo, hi in ((0, 1), (1, 65), (0, len(lens))):
            got, exp = rig.step(hdr[lo:hi], lens[lo:hi], outs=SEP if hi - lo > 64 else PART)
        assert ((exp["verdict"] & 0xFF) == ST["PORTSCAN_DROP"]).any()
    finally:
        rig.close()

