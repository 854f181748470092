"""The land, SYN-flood and UDP-flood monitors on the stateless classify path (ppe_attack_*) on the GPU, exact against the
oracle's result rewritten by the tests' serial model (tests/attack_model.py, composed with tests/portscan_model.py and
tests/stream_model.py): verdict word, ACL hit, flow hash, tuple, the lists of every result layout, ppe_counters_t, the
stream counters and ppe_attack_info (all four ports' ten state fields and the four drop totals), after every batch and
every tick.  Every output buffer carries 64 guard entries behind its last one, which must stay untouched.

Integer work: no tolerance anywhere."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import attack_model as am  # noqa: E402
import decode_corpus as dc  # noqa: E402
import pyoracle  # noqa: E402
import stream_model as sm  # noqa: E402
from attack_model import AttackModel, batch, frame  # noqa: E402
from portscan_model import PortScanModel  # noqa: E402
from ppe import Engine, PPEError, abi, synth  # noqa: E402
from ppe.abi import ST  # noqa: E402

NOW = 1_700_000_000
DEV = torch.device("cuda:0")
GUARD = 64
SEP = ("verdict", "flow_hash", "acl_hit", "fw_idx", "drop_idx", "tile_cnt", "tuple")
PART = ("verdict", "flow_hash", "acl_hit", "part_idx")
PART8 = ("verdict", "flow_hash", "acl_hit", "part8")
PACKED = ("packed", "part8")
PLAIN = ("verdict", "flow_hash", "acl_hit", "tuple")
LAYOUTS = (SEP, PART, PART8, PACKED, PLAIN)
LAND, SYNF, SYNC, UDPF = ST["ATTACK_LAND"], ST["ATTACK_SYNFLOOD"], ST["ATTACK_SYNCOUNT"], ST["ATTACK_UDPFLOOD"]
A, B = 0x0A000001, 0x0B000002
STREAM_ON = (1, 0, 0)
# port 0: land and both floods at speed 0 (any traffic arms the next interval); port 1: land off (2), floods at a
# threshold; port 2: everything on but drop_pack 2 (nothing drops); port 3: the count monitor alone
PD = {0: dict(drop_pack=1, land=1), 1: dict(drop_pack=1, land=2), 2: dict(drop_pack=2, land=1), 3: dict(drop_pack=1)}
TD = {0: dict(drop_pack=1, flood_udp=1, udp_speed=0, flood_syn=1, syn_speed=0, syn_count=1 << 30),
      1: dict(drop_pack=1, flood_udp=1, udp_speed=5, flood_syn=1, syn_speed=3, syn_count=1 << 30),
      2: dict(drop_pack=2, flood_udp=1, udp_speed=0, flood_syn=1, syn_speed=0, syn_count=0),
      3: dict(drop_pack=1, flood_udp=0, udp_speed=0, flood_syn=2, syn_speed=0, syn_count=2)}


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
        if getattr(e, "attack_attached", None) is not None:
            e.attack_attached.close()
        if getattr(e, "portscan_attached", None) is not None:
            e.portscan_attached.close()
        e.stream_tcp(0, 0, 0)


def no_rules():
    return np.zeros(0, abi.RULE_DTYPE)


def alloc(n, outs):
    shapes = {"tile_cnt": (n + 63) // 64, "tuple": 4 * n}
    out = {k: torch.full((shapes.get(k, n) + GUARD,), -7, dtype=torch.int32, device=DEV) for k in outs
           if k not in ("part8", "packed")}
    if "part8" in outs:
        out["part8"] = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    if "packed" in outs:
        out["packed"] = torch.full((n + GUARD,), -7, dtype=torch.int64, device=DEV)
    return out


def collect(out, n):
    """Host copies of the outputs, their guard entries checked and cut off."""
    sizes = {"tile_cnt": (n + 63) // 64, "tuple": 4 * n}
    res = {}
    for k, v in out.items():
        a, m = v.cpu().numpy(), sizes.get(k, n)
        fill = 0xEE if k == "part8" else -7
        assert (a[m:] == fill).all() and len(a) == m + GUARD, f"{k}: guard entries written"
        a = a[:m]
        res[k] = a if k in ("acl_hit", "part8") else a.view(np.uint64) if k == "packed" else a.view(np.uint32)
    if "tuple" in res:
        res["tuple"] = res["tuple"].reshape(n, 4)
    if "packed" in res:
        res.update(abi.unpack(res["packed"]))
    return res


def compare(got, exp, n, what="", tmask=None):
    """tmask: decode_corpus.expected's tuple_mask (of a frame punted at the window only addresses and protocol are
    defined)."""
    for k in ("verdict", "flow_hash", "acl_hit") + (("tuple",) if "tuple" in got else ()):
        g = got[k] & tmask if k == "tuple" and tmask is not None else got[k]
        bad = np.flatnonzero((g != exp[k]).reshape(n, -1).any(axis=1))
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:4]], exp[k][bad[:4]])
    if "packed" in got:
        assert np.array_equal(got["packed"], sm.packed(exp["verdict"], exp["flow_hash"], exp["acl_hit"])), what
    want = sm.lists(exp["verdict"])
    for k in ("fw_idx", "drop_idx", "tile_cnt", "part_idx", "part8"):
        if k in got:
            assert np.array_equal(got[k], want[k]), (what, k)


def to_dev(hdr, lens, ports=None):
    th = torch.from_numpy(np.ascontiguousarray(hdr)).to(DEV)
    tl = torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32)).to(DEV)
    tp = torch.from_numpy(np.ascontiguousarray(ports, np.uint8)).to(DEV) if ports is not None else None
    return th, tl, tp


class Rig:
    """An engine with the monitors attached, the serial model beside it (with the port-scan and StreamTcp models when
    those are on) and the oracle for the rule set: step() runs one batch through both and compares everything."""

    def __init__(self, eng, rules=None, default_action=abi.ACL_RULE_ACTION_FW, pd=None, td=None, hold=600, stream=None,
                 syn_check=1, portscan=None, commit=True):
        self.eng, self.syn_check, self.stream = eng, syn_check, stream
        self.rules = no_rules() if rules is None else rules
        self.default_action = default_action
        if commit:
            eng.commit(self.rules, default_action=default_action)
        eng.stream_tcp(*(stream or (0, 0, 0)))
        self.m = AttackModel(pd, td, hold)
        self.atk = eng.attack(self.m.cfg())
        self.ps = self.pm = None
        if portscan is not None:
            d = dict(exception_freq=3, hold_seconds=600, capacity=1 << 16, max_batch=8192, cycles_per_second=1000)
            d.update(portscan)
            self.ps = eng.portscan(**d)
            self.pm = PortScanModel(**{k: v for k, v in d.items() if k != "max_batch"})
            self.ps.clock(50_000, NOW)
            self.pm.clock(50_000, NOW)
        self.clock(NOW)

    @property
    def oracle(self):
        return pyoracle.Oracle(self.rules, default_action=self.default_action)

    def clock(self, now):
        self.atk.clock(now)
        self.m.clock(now)

    def tick(self, now):
        self.atk.tick(now)
        self.m.tick(now)
        self.check_info("after a tick")

    def set(self, pd=None, td=None, hold=600):
        self.m.set(pd, td, hold)
        self.atk.set(self.m.cfg())

    def close(self):
        self.atk.close()
        if self.ps is not None:
            self.ps.close()

    def reference(self, hdr, lens):
        o = self.oracle
        return o.classify_batch(hdr, lens, cfg=o.cfg(0, self.syn_check, NOW))

    def expected(self, ref, hdr, ports):
        sc = dict(zip(("track", "midstream", "async_oneside"), self.stream or (0, 0, 0)))
        return self.m.expected(ref, hdr, ports, portscan=self.pm, now_seconds=NOW, stream=sc)

    def classify(self, hdr, lens, ports, outs):
        n = len(lens)
        th, tl, tp = to_dev(hdr, lens, ports)
        self.atk.ports([tp] if tp is not None else None)
        out = alloc(n, outs)
        self.eng.classify_torch(th, tl, out, cfg=self.eng.cfg(0, self.syn_check, NOW))
        torch.cuda.synchronize()
        return collect(out, n)

    def step(self, hdr, lens, ports=None, outs=PLAIN, ref=None, what="", tmask=None):
        n = len(lens)
        self.eng.clear_counters()
        self.eng.clear_stream_counters()
        if ref is None:
            ref = self.reference(hdr, lens)
        exp = self.expected(ref, hdr, ports)
        got = self.classify(hdr, lens, ports, outs)
        compare(got, exp, n, what, tmask)
        assert self.eng.counters() == exp["counters"], what
        assert self.eng.stream_counters() == exp["stream"], what
        self.check_info(what)
        if self.ps is not None:
            assert {tuple(int(x) for x in e) for e in self.ps.dump()} == self.pm.records(), what
        return got, exp

    def check_info(self, what=""):
        info, want = self.atk.info(), self.m.info()
        for p in range(4):
            g = {k: info["ai"][p][k] for k in abi.ATTACK_STATE_FIELDS}
            assert g == want["ai"][p], (what, "port", p, g, want["ai"][p])
        assert {k: info[k] for k in abi.ATTACK_TOTALS} == {k: want[k] for k in abi.ATTACK_TOTALS}, what


def mixed(n, seed, only_last=None):
    """n frames of every class with ports 0-3 mixed inside every tile; every fifth TCP / UDP frame has sip == dip and
    every third a VLAN tag.  only_last: every frame but the last is one no monitor judges, the last of that kind."""
    rng = np.random.default_rng(seed)
    kinds = rng.choice(np.array(("udp", "udp", "udp_short", "udp_lenerr", "syn", "syn", "synack", "ack", "syn_lenerr",
                                 "frag", "icmp", "rst")), n)
    if only_last:
        kinds[:] = "icmp"
        kinds[-1] = only_last
    fr = [frame(k, A + i, A + i if i % 5 == 0 and not only_last else B, vlan_tag=i % 3 == 0, dport=80 + i % 7)
          for i, k in enumerate(kinds)]
    ports = rng.integers(0, 4, n).astype(np.uint8)
    return batch(fr) + (ports,)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_known_answers(eng, n):
    """The CPU known answers (tests/test_attack.py) as batches with tail lanes: enable words 0 / 1 / 2, drop_pack on both
    halves, strict thresholds, land only on TCP SYN and outside syn_accum, a short UDP header under a flood, the hold
    set once with its launch's clock and cleared by the tick at hold_time, independent ports.  In one batch only the
    last valid lane is of the arming class."""
    rig = Rig(eng, pd=PD, td=TD, hold=2, syn_check=1)
    seen = set()
    for sec in range(6):
        for sub in range(2):
            rig.clock(NOW + sec + 10 * sub)        # (a later clock in the same interval does not move a hold)
            hdr, lens, ports = mixed(n if sec < 4 else max(1, n // 16), 100 * n + 10 * sec + sub)
            _, exp = rig.step(hdr, lens, ports, outs=LAYOUTS[(sec + sub) % 5], what=f"n {n} sec {sec}.{sub}")
            seen |= set((exp["verdict"] & 0xFF).tolist())
        rig.tick(NOW + sec + 1)
    if n >= 63:
        assert {LAND, SYNF, SYNC, UDPF} <= seen, seen
    # only the last valid lane arms: port 0's UDP hold, then its SYN hold, each with this launch's clock
    rig.set(PD, TD, hold=7)
    for kind, field in (("udp", "udp_flood_hold"), ("syn", "syn_flood_hold")):
        rig.tick(NOW + 100)
        rig.tick(NOW + 100)                         # two quiet ticks: every pps 0, every hold released
        assert all(a[field] == 0 for a in rig.m.ai)
        hdr, lens, _ = mixed(n, 7, only_last=kind)
        ports = np.zeros(n, np.uint8)
        rig.step(hdr, lens, ports)                  # pps was 0: counted, not dropped
        rig.tick(NOW + 101)
        rig.clock(NOW + 103)
        _, exp = rig.step(hdr, lens, ports, outs=SEP)
        assert int(exp["verdict"][-1]) & 0xFF == (UDPF if kind == "udp" else SYNF)
        assert rig.m.ai[0][field] == 1 and rig.m.ai[0][field + "_time"] == NOW + 110
    rig.close()


def test_strict_thresholds_on_the_device(eng):
    """One deterministic batch on each side of every comparator of the decision word: pps == speed passes and
    speed + 1 drops (UDP on port 1, SYN on port 2), syncount == syn_count passes and + 1 drops with flood_syn 0
    (port 3).  The counts are preloaded through ticks; the statuses below are worked out by hand, not by the model."""
    td = {1: dict(drop_pack=1, flood_udp=1, udp_speed=7), 2: dict(drop_pack=1, flood_syn=1, syn_speed=7, syn_count=1 << 30),
          3: dict(drop_pack=1, flood_syn=0, syn_count=5)}
    rig = Rig(eng, td=td, hold=50)

    def run(nu, ns, nc):
        fr = [frame("udp", A + i, B) for i in range(nu)] + [frame("syn", A + i, B) for i in range(ns + nc)]
        hdr, lens = batch(fr)
        ports = np.array([1] * nu + [2] * ns + [3] * nc, np.uint8)
        _, exp = rig.step(hdr, lens, ports, outs=SEP)
        st = (exp["verdict"] & 0xFF).tolist()
        return set(st[:nu]), set(st[nu:nu + ns]), set(st[nu + ns:])
    fw = {ST["ACL_FW"]}
    assert run(7, 7, 5) == (fw, fw, fw)                 # every count 0 so far
    rig.tick(NOW + 1)                                   # udppps 7, synpps 7, syncount 5: each equal to its threshold
    assert [rig.m.ai[1]["udppps"], rig.m.ai[2]["synpps"], rig.m.ai[3]["syncount"]] == [7, 7, 5]
    assert run(8, 8, 6) == (fw, fw, fw)                 # equal passes
    assert rig.atk.info()["ai"][1]["udp_flood_hold"] == 0 and rig.atk.info()["ai"][2]["syn_flood_hold"] == 0
    rig.tick(NOW + 2)                                   # 8, 8, 6: each one above
    assert run(3, 3, 3) == ({UDPF}, {SYNF}, {SYNC})
    info = rig.atk.info()
    assert (info["udpflood_drop"], info["synflood_drop"], info["syncount_drop"], info["land_drop"]) == (3, 3, 3, 0)
    assert info["ai"][1]["udp_flood_hold_time"] == NOW + 52 and info["ai"][2]["syn_flood_hold_time"] == NOW + 52
    assert info["ai"][3]["syn_flood_hold"] == 0 and info["ai"][3]["syncount_accum"] == 0
    rig.tick(NOW + 3)                                   # pps 3, 3 but held; syncount 0: the count monitor lets go
    assert run(2, 2, 2) == ({UDPF}, {SYNF}, fw)
    rig.close()


def sweep_batch():
    """synth.make_tcp_flag_sweep (all 64 flag values x plain / VLAN / ihl 6, UDP good and malformed) with every other
    sweep packet's dip set to its sip, plus fragments and frames whose L4 header lies past a 64-B window."""
    rules = synth.make_rules(256, seed=256)
    pk = synth.make_tcp_flag_sweep(rules, stride=256)
    hdr, lens = pk["hdr"].copy(), pk["len"].copy()
    for i in np.flatnonzero(pk["layout"] >= 0)[::2]:
        l3 = 18 if pk["layout"][i] == 1 else 14
        hdr[i, l3 + 16:l3 + 20] = hdr[i, l3 + 12:l3 + 16]
    extra = [frame(k, A + i, A + i if i & 1 else B, vlan_tag=bool(i & 2), ihl=ihl)
             for i, (k, ihl) in enumerate([("frag", 5), ("frag", 6), ("syn", 15), ("udp", 15), ("syn", 11), ("udp", 12),
                                           ("udp_short", 15), ("synack", 13)] * 4)]
    eh, el = batch(extra, stride=256)
    hdr, lens = np.concatenate([hdr, eh]), np.concatenate([lens, el])
    ports = (np.arange(len(lens)) * 7 % 4).astype(np.uint8)
    return rules, hdr, lens, ports


@pytest.mark.parametrize("stream", [None, STREAM_ON], ids=["plain", "stream"])
@pytest.mark.parametrize("syn_check", [1, 0])
def test_flag_sweep_over_three_intervals(eng, stream, syn_check):
    """Below threshold -> arming -> held -> released, over the flag sweep at a 64-B window."""
    rules, hdr, lens, ports = sweep_batch()
    rig = Rig(eng, rules, abi.ACL_RULE_ACTION_DROP, pd=PD, td=TD, hold=2, stream=stream, syn_check=syn_check)
    o = rig.oracle

    def window64(sl):
        e = dc.expected(o, hdr[sl], lens[sl], 64, o.cfg(0, syn_check, NOW))
        return {k: e[k] for k in ("verdict", "flow_hash", "acl_hit", "tuple", "counters")}, e["tuple_mask"]
    full, quiet = window64(slice(None)), window64(slice(0, 37))   # the last intervals carry a tile's worth: the floods end
    st = full[0]["verdict"] & 0xFF
    assert (st == ST["WINDOW_PUNT"]).sum() >= 8 and (st == ST["FRAG"]).sum() >= 8
    held = []
    for sec, outs in enumerate((SEP, PART8, PACKED, PLAIN, PART, SEP)):
        sl = slice(0, 37) if sec >= 3 else slice(None)
        ref, tmask = quiet if sec >= 3 else full
        rig.clock(NOW + sec)
        rig.step(np.ascontiguousarray(hdr[sl, :64]), lens[sl], ports[sl], outs=outs, ref=ref, what=f"sec {sec}",
                 tmask=tmask)
        held.append(rig.m.ai[0]["udp_flood_hold"] + rig.m.ai[0]["syn_flood_hold"])
        rig.tick(NOW + sec + 1)
    assert held[0] == 0 and held[1] == 2 and held[2] == 2 and rig.m.ai[0]["udp_flood_hold"] == 0
    assert all(rig.m.totals[k] > 0 for k in abi.ATTACK_TOTALS)
    rig.close()


# one (rule count, tuning) per fetch x placement family ppe_launch_info reports (tests/test_gpu_decode_edges.py TUNINGS)
FAMILIES = [(256, dict(), ("hoist", "lds")), (4096, dict(), ("cut", "lds")),
            (256, dict(lds_image=0), ("multi", "global")), (256, dict(pipeline=1), ("none", "lds")),
            (4096, dict(pipeline=1), ("none", "split")), (256, dict(pipeline=3), ("multi", "lds")),
            (4096, dict(pipeline=4), ("hoist", "split")), (256, dict(pipeline=5, lds_image=0), ("cut", "global")),
            (4096, dict(pipeline=5, block=256), ("cut", "split"))]
_size = {}


def size_world(nrules):
    """4,096 + 37 packets (several workgroups, a tail tile), their ports and the oracle's answer, once per rule set."""
    if nrules not in _size:
        rules = synth.make_rules(nrules, seed=nrules)
        pk = synth.make_packets(4096 + 37, rules, seed=5, kind="imix", stride=128, malformed_frac=0.08, tcp_frac=0.5)
        hdr, lens = pk["hdr"].copy(), pk["len"].copy()
        for i in range(0, len(lens), 6):               # some land packets (untagged, ihl 5 rows only)
            if hdr[i, 12] == 0x08 and hdr[i, 14] == 0x45:
                hdr[i, 30:34] = hdr[i, 26:30]
        ports = np.random.default_rng(9).integers(0, 4, len(lens)).astype(np.uint8)
        o = pyoracle.Oracle(rules, default_action=abi.ACL_RULE_ACTION_FW)
        _size[nrules] = (rules, hdr, lens, ports, o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW)))
    return _size[nrules]


@pytest.mark.parametrize("nrules,tune,family", FAMILIES, ids=["-".join(f[2]) for f in FAMILIES])
def test_every_family_and_layout_across_workgroups(eng, nrules, tune, family):
    """4,133 packets over every fetch x placement family, every result layout, with the monitors alone and together
    with StreamTcp and the port-scan table: the per-port sums come from several workgroups, and in the arming interval
    several workgroups race for each hold."""
    rules, hdr, lens, ports, ref = size_world(nrules)
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
    old = eng.tuning()
    try:
        eng.tuning(**tune)
        info = eng.launch_info()
        assert (info["fetch"], info["image"]) == family, (tune, info)
        for stream, portscan in ((None, None), (STREAM_ON, None), (None, {}), (STREAM_ON, {})):
            rig = Rig(eng, rules, pd=PD, td=TD, hold=1, stream=stream, portscan=portscan, commit=False)
            for sec, outs in enumerate(LAYOUTS):
                rig.clock(NOW + sec)
                rig.step(hdr, lens, ports, outs=outs, ref=ref, what=f"{family} {stream} {portscan} sec {sec}")
                if sec in (0, 2):
                    rig.tick(NOW + sec + 1)
            assert all(rig.m.totals[k] > 0 for k in abi.ATTACK_TOTALS)
            assert rig.m.ai[0]["udp_flood_hold"] == 1 and rig.m.ai[1]["syn_flood_hold"] == 1
            rig.close()
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("stride", [64, 144])
def test_decode_edge_corpus(eng, stride):
    """The decode edge corpus with all-zero rules attached: byte-identical to a context with nothing attached, the
    accumulators equal to the model's; then with land and both floods dropping."""
    rules = synth.make_rules(256, seed=256)
    hdr256, lens, _ = dc.corpus(rules)
    hdr256 = hdr256.copy()
    for i in range(0, len(lens), 7):                   # some land frames (untagged, ihl 5 rows only)
        if hdr256[i, 12] == 0x08 and hdr256[i, 13] == 0x00 and hdr256[i, 14] == 0x45:
            hdr256[i, 30:34] = hdr256[i, 26:30]
    hdr = np.ascontiguousarray(hdr256[:, :stride])
    n = len(lens)
    eng.commit(rules, default_action=1)
    o = pyoracle.Oracle(rules, default_action=1)
    e = dc.expected(o, hdr256, lens, stride, o.cfg(0, 1, NOW))
    ref, tmask = {k: e[k] for k in ("verdict", "flow_hash", "acl_hit", "tuple", "counters")}, e["tuple_mask"]
    th, tl, _ = to_dev(hdr, lens)
    eng.clear_counters()
    out = alloc(n, SEP)
    eng.classify_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
    torch.cuda.synchronize()
    base, base_cnt = collect(out, n), eng.counters()
    ports = (np.arange(n) % 4).astype(np.uint8)
    rig = Rig(eng, rules, 1, commit=False)
    got, _ = rig.step(hdr, lens, ports, outs=SEP, ref=ref, what="all-zero rules", tmask=tmask)
    for k in SEP:
        assert np.array_equal(got[k], base[k]), k
    assert eng.counters() == base_cnt
    assert sum(a["udp_accum"] + a["syn_accum"] for a in rig.m.ai) > 100 and not any(rig.m.totals.values())
    on = dict(drop_pack=1, flood_udp=1, udp_speed=0, flood_syn=1, syn_speed=0, syn_count=1 << 30)
    rig.set({p: dict(drop_pack=1, land=1) for p in range(4)}, {p: on for p in range(4)}, hold=5)
    rig.tick(NOW + 1)
    for outs in (SEP, PACKED):
        _, exp = rig.step(hdr, lens, ports, outs=outs, ref=ref, what="everything dropping", tmask=tmask)
    st = exp["verdict"] & 0xFF
    assert (st == LAND).any() and (st == SYNF).any() and (st == UDPF).any()
    rig.close()


def scanner(n, land_every=3):
    """One source walking the ports (a scanner), TCP SYN; every land_every-th frame has sip == dip == the scanner."""
    fr = [frame("syn", A, A if i % land_every == 0 else B, dport=1000 + i) for i in range(n)]
    fr += [frame("synack", B, A, dport=99), frame("udp", A, B, dport=5), frame("ack", A, B)]
    return batch(fr)


@pytest.mark.parametrize("stream", [None, STREAM_ON], ids=["plain", "stream"])
def test_with_the_portscan_table(eng, stream):
    """A scanner whose SYNs are land- or flood-dropped does not advance its record: the dumped records equal the
    composed model's.  With StreamTcp's defaults a SYN|ACK is counted in syncount_accum, then dropped as 22."""
    hdr, lens = scanner(120)
    rig = Rig(eng, pd={0: dict(land=1, drop_pack=1)}, td={0: dict(flood_syn=1, syn_speed=50, syn_count=1 << 30, drop_pack=1)},
              hold=3, stream=stream, portscan=dict(exception_freq=0, capacity=64))
    _, e0 = rig.step(hdr, lens, what="land only")
    st = e0["verdict"] & 0xFF
    assert (st == LAND).sum() == 40 and (st == ST["PORTSCAN_DROP"]).any()
    if stream:
        assert int(st[120]) == ST["STREAM_MIDSTREAM_ONESIDE_OFF"]
    need = abi.F_TCP | abi.F_SYN
    fwd = np.isin(st, (ST["ACL_FW"], ST["STREAM_MIDSTREAM_ONESIDE_OFF"])) & (((e0["verdict"] >> 16) & need) == need)
    assert rig.m.ai[0]["syncount_accum"] == int(fwd.sum()) >= 1      # port-scan drops are not in it, StreamTcp's are
    mine = lambda recs: {r for r in recs if r[0] == A}  # noqa: E731
    before = mine(rig.pm.records())
    rig.tick(NOW + 1)                                   # synpps 81 > 50: every SYN is flood-dropped from here on
    _, e1 = rig.step(hdr, lens, what="flood")
    st = e1["verdict"] & 0xFF
    assert (st == SYNF).sum() == 81 and (st == LAND).sum() == 40 and not (st[:121] == ST["PORTSCAN_DROP"]).any()
    assert len(before) == len(mine(rig.pm.records())) == 1   # one record for the scanner, before and after
    rig.close()


def batches_call(eng, rig, specs, ports_for):
    """One ppe_classify_batches call over the (hdr, lens, ports) of specs (an entry None: an empty batch); returns the
    per-batch results.  ports_for(k, ports) picks what batch k's entry of ppe_attack_ports is."""
    K = len(specs)
    bats, ress, keep, parr = [], [], [], []
    for k, sp in enumerate(specs):
        if sp is None:
            bats.append(abi.Batch(None, None, None, 0, 64))
            ress.append(abi.Result())
            keep.append(None)
            parr.append(None)
            continue
        hdr, lens, ports = sp
        th, tl, tp = to_dev(hdr, lens, ports_for(k, ports))
        out = alloc(len(lens), PLAIN)
        bats.append(abi.Batch(th.data_ptr(), tl.data_ptr(), None, len(lens), hdr.shape[1]))
        ress.append(abi.Result(out["verdict"].data_ptr(), out["flow_hash"].data_ptr(), out["acl_hit"].data_ptr(), None,
                               None, None, out["tuple"].data_ptr()))
        keep.append((th, tl, tp, out))
        parr.append(tp)
    rig.atk.ports(parr)
    ins, outs = (abi.Batch * K)(*bats), (abi.Result * K)(*ress)
    cfg = eng.cfg(0, 1, NOW)
    s = torch.cuda.current_stream(DEV)
    assert eng.lib.ppe_classify_batches(eng.ctx, ins, outs, K, C.byref(cfg), C.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    return [collect(k[3], len(sp[1])) if k is not None else None for k, sp in zip(keep, specs)]


@pytest.mark.parametrize("K", [3, 34])
def test_classify_batches(eng, K):
    """3 batches (kernel-argument descriptors) and 34 (the descriptor ring), per-batch port arrays with one of them
    NULL (port 0) and, among the 34, an empty batch, which must not shift the arrays; one clock per call."""
    rig = Rig(eng, pd=PD, td=TD, hold=4)
    sizes = (65, 1, 129, 257, 64, 37)
    for call in range(3):
        specs = [mixed(sizes[(k + call) % 6], 1000 * call + k) for k in range(K)]
        if K == 34:
            specs[5] = None
        null_at = 1 if K == 3 else 17
        rig.clock(NOW + call)
        eng.clear_counters()
        total = dict.fromkeys(abi.COUNTERS, 0)
        exps = []
        for k, sp in enumerate(specs):
            if sp is None:
                exps.append(None)
                continue
            hdr, lens, ports = sp
            e = rig.expected(rig.reference(hdr, lens), hdr, None if k == null_at else ports)
            exps.append(e)
            for c, v in e["counters"].items():
                total[c] += v
        got = batches_call(eng, rig, specs, lambda k, p: None if k == null_at else p)
        for k, (g, e) in enumerate(zip(got, exps)):
            if e is not None:
                compare(g, e, len(specs[k][1]), f"call {call} batch {k}")
        assert eng.counters() == total
        rig.check_info(f"call {call}")
        rig.tick(NOW + call + 1)
    assert all(rig.m.totals[k] > 0 for k in abi.ATTACK_TOTALS)
    rig.close()


def test_set_and_tick_are_stream_ordered(eng):
    """ppe_attack_set and ppe_attack_tick enqueued between queued batches, no synchronise in between: each takes effect
    exactly at its place in the stream."""
    rig = Rig(eng, hold=9)
    hdr, lens, ports = mixed(257, 3)
    th, tl, tp = to_dev(hdr, lens, ports)
    rig.atk.ports([tp])
    ref = rig.reference(hdr, lens)
    eng.clear_counters()
    outs, exps = [], []

    def enqueue():
        out = alloc(len(lens), PLAIN)
        eng.classify_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
        outs.append(out)
        exps.append(rig.expected(ref, hdr, ports))
    enqueue()                                           # all-zero rules: only the accumulators move
    rig.set(PD, TD, hold=9)
    enqueue()                                           # rules on, pps still 0: land drops only
    rig.tick(NOW + 1)
    enqueue()                                           # arming
    rig.set(PD, {p: dict(TD[p], drop_pack=0) for p in TD}, hold=9)
    enqueue()                                           # traffic half off: land only, the holds stay
    rig.tick(NOW + 2)
    rig.set(PD, TD, hold=9)
    enqueue()                                           # held
    rig.tick(NOW + 10)                                  # hold_time = NOW + 10: released, pps of one batch
    enqueue()
    torch.cuda.synchronize()
    total = dict.fromkeys(abi.COUNTERS, 0)
    kinds = []
    for i, (out, e) in enumerate(zip(outs, exps)):
        compare(collect(out, len(lens)), e, len(lens), f"launch {i}")
        kinds.append(set((e["verdict"] & 0xFF).tolist()) & {LAND, SYNF, SYNC, UDPF})
        for c, v in e["counters"].items():
            total[c] += v
    assert kinds[0] == set() and kinds[1] == {LAND} and {SYNF, UDPF} <= kinds[2] and kinds[3] == {LAND}
    assert {SYNF, UDPF} <= kinds[4]
    assert eng.counters() == total
    rig.check_info()
    rig.atk.clear_stat()
    rig.m.totals = dict.fromkeys(abi.ATTACK_TOTALS, 0)  # the four drop totals only
    rig.check_info("after clear_stat")
    rig.close()


def test_detach_refusals_and_port_mask(eng):
    """Attached then detached: byte-identical to never attached.  PPE_ENOTSUP from ppe_classify_flow, ppe_classify_host
    and the steered path with the monitors attached; nothing is touched and the flow table works afterwards.  Ports
    >= 4 behave as port & 3."""
    rules = synth.make_rules(256, seed=256)
    pk = synth.make_flow_packets(4096, rules, n_flows=600, seed=21, syn_frac=0.6)
    hdr, lens = pk["hdr"], pk["len"]
    eng.commit(rules, default_action=abi.ACL_RULE_ACTION_FW)
    th, tl, _ = to_dev(hdr, lens)

    def plain_run():
        eng.clear_counters()
        out = alloc(4096, SEP)
        eng.classify_torch(th, tl, out, cfg=eng.cfg(0, 1, NOW))
        torch.cuda.synchronize()
        return collect(out, 4096), eng.counters()
    base, base_cnt = plain_run()
    rig = Rig(eng, rules, pd=PD, td=TD, commit=False)
    rig.step(hdr, lens, (np.arange(4096) % 4).astype(np.uint8))
    rig.atk.detach()
    got, cnt = plain_run()
    for k in SEP:
        assert np.array_equal(got[k], base[k]), k
    assert cnt == base_cnt
    rig.atk.attach()
    lib = eng.lib
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
        before = rig.atk.info()
        assert lib.ppe_classify_flow(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg), s) == abi.PPE_ENOTSUP
        hv = np.full(256, 0xFFFFFFF9, np.uint32)
        hh, hl = hdr[:256].copy(), lens[:256].copy()
        hb = abi.Batch(hh.ctypes.data, hl.ctypes.data, None, 256, 64)
        hr = abi.Result(hv.ctypes.data, None, None, None, None, None, None)
        assert lib.ppe_classify_host(eng.ctx, C.byref(hb), C.byref(hr), C.byref(cfg), 0) == abi.PPE_ENOTSUP
        from ppe.dist import DeviceSteerOps, steered_classify_flow
        with pytest.raises(PPEError, match="-95"):      # before any collective: no process group is needed to see it
            steered_classify_flow(DeviceSteerOps(eng), None, th, tl, cfg, 1, 0)
        torch.cuda.synchronize()
        assert (out["verdict"].cpu().numpy() == -7).all() and (hv == 0xFFFFFFF9).all()   # nothing ran
        assert eng.flow_info()["live"] == 0 and rig.atk.info() == before
        rig.step(hdr, lens, (np.arange(4096) % 4).astype(np.uint8))       # the monitors work
        rig.atk.detach()
        eng.classify_flow_torch(th, tl, out, cfg=cfg)                     # and so does the flow table
        torch.cuda.synchronize()
        ref = ft.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW))
        assert np.array_equal(out["verdict"].cpu().numpy().view(np.uint32), ref["verdict"])
        assert eng.flow_info()["live"] == ft.stats()["live"] > 0
        assert lib.ppe_classify_host(eng.ctx, C.byref(hb), C.byref(hr), C.byref(cfg), 0) == 0
    finally:
        eng.flow_destroy()
        rig.close()
    # ports >= 4: the kernel takes port & 3 (the model does the same); nothing is indexed past four ports
    rig = Rig(eng, pd=PD, td=TD)
    h2, l2, p2 = mixed(257, 11)
    wild = (p2.astype(np.uint32) + 4 * (np.arange(257) % 63)).astype(np.uint8)
    assert (wild >= 4).sum() > 200 and np.array_equal(wild & 3, p2)
    rig.step(h2, l2, wild)
    rig.tick(NOW + 1)
    rig.step(h2, l2, wild, outs=SEP)
    assert any(rig.m.totals.values())
    rig.close()


def test_show_text_from_a_live_object(eng):
    """ppe_format_attack_stat of ppe_attack_info's struct prints the rules in force and the state the model holds."""
    rig = Rig(eng, pd=PD, td=TD, hold=30)
    hdr, lens, ports = mixed(129, 1)
    rig.step(hdr, lens, ports)
    rig.tick(NOW + 1)
    info = rig.atk.info_struct()
    n = eng.lib.ppe_format_attack_stat(C.byref(info), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert eng.lib.ppe_format_attack_stat(C.byref(info), buf, n + 1) == n
    text = buf.value.decode()
    for p in range(4):
        assert f"interface {p}:\n" in text and f"udppps: {rig.m.ai[p]['udppps']}\n" in text
    assert "syn_count: 1073741824\n" in text and rig.atk.info()["cfg"]["hold_seconds"] == 30
    rig.close()
