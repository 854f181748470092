"""The decode edge corpus (tests/decode_corpus.py) through the stateless classify path on the GPU: every kernel family
and image placement, every result layout, header windows on both sides of the window rule (64 and 80 punt, 96 to 256
do not), batch tails, residual MAC / time rules and mixed ring calls.

Bar: bit-exact against decode_corpus.expected (the oracle on the 256-B window; the whole WINDOW_PUNT verdict word,
flow hash 0 and hit -1 for a frame that does not fit the window), the 32 counters exactly, and every output tensor's
64 guard entries past n untouched.  The inputs carry 320 rows of 0xA5 past n, so a lane past the end of a batch stays
inside the test's own tensors whatever index it reads by."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import pyoracle  # noqa: E402
from ppe import Engine, abi, synth  # noqa: E402

import decode_corpus as dc  # noqa: E402
from test_gpu_parity import check_compaction, check_part8, check_partition  # noqa: E402

NOW = 1_700_000_000
DEV = torch.device("cuda:0")
GUARD, PAST = 64, 320
STRIDES = (64, 80, 96, 128, 144, 256)
RULESETS = {256: dict(seed=256), 4096: dict(seed=4096), 300: dict(seed=70, resid_frac=0.3)}
LAYOUTS = ("soa", "part", "part8", "packed")

# tuning -> (fetch, image placement) ppe_launch_info must report for the 256- and the 4,096-rule image (what the
# host-only planner decides for them: a silent fallback to another kernel family fails the sweep)
TUNINGS = [
    (dict(), ("hoist", "lds"), ("cut", "lds")),
    (dict(lds_image=0), ("multi", "global"), ("multi", "global")),
    (dict(pipeline=1), ("none", "lds"), ("none", "split")),
    (dict(pipeline=3), ("multi", "lds"), ("multi", "lds")),
    (dict(pipeline=3, lds_image=0), ("multi", "global"), ("multi", "global")),
    (dict(pipeline=4), ("hoist", "lds"), ("hoist", "split")),
    (dict(pipeline=5, lds_image=0), ("cut", "global"), ("cut", "global")),
    (dict(pipeline=5, block=256), ("cut", "lds"), ("cut", "split")),
    (dict(block=1024), ("hoist", "lds"), ("hoist", "split")),
]
_families = {f for _, a, b in TUNINGS for f in (a, b)}
assert {f for f, _ in _families} == {"hoist", "none", "multi", "cut"}
assert {i for _, i in _families} == {"lds", "split", "global"}


def tune_id(t):
    return ",".join(f"{k}={v}" for k, v in t.items()) or "default"


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


class World:
    """One rule set's corpus, its device copies per stride and the oracle's answers, each computed once."""

    def __init__(self, nrules):
        self.rules = synth.make_rules(nrules, **RULESETS[nrules])
        self.hdr, self.lens, self.meta = dc.corpus(self.rules)
        self.n = len(self.lens)
        if nrules == 300:
            aim_macs(self.rules, self.hdr, self.lens)
        self.ts = None
        self._wide, self._exp, self._dev = {}, {}, {}

    @property
    def oracle(self):
        """(the C oracle holds one rule set at a time: set again before every use)"""
        return pyoracle.Oracle(self.rules, default_action=1)

    def expected(self, stride, syn=1, unsup=0):
        key = (stride, syn, unsup)
        if key not in self._exp:
            oracle = self.oracle
            cfg = oracle.cfg(unsup, syn, NOW)
            if key[1:] not in self._wide:
                self._wide[key[1:]] = oracle.classify_batch(self.hdr, self.lens, ts=self.ts, cfg=cfg)
            self._exp[key] = dc.expected(oracle, self.hdr, self.lens, stride, cfg, ts=self.ts,
                                         wide=self._wide[key[1:]])
        return self._exp[key]

    def device(self, stride):
        if stride not in self._dev:
            self._dev[stride] = to_device(self.hdr[:, :stride], self.lens, self.ts)
        return self._dev[stride]


def aim_macs(rules, hdr, lens):
    """synth draws the MACs of its rules and of its packets from two different pools, so a MAC rule never matches a
    synth packet: the window's MAC bytes are read and compared, but a wrong read would compare unequal all the same.
    Here every MAC rule takes the MACs of the first corpus frame inside its box (addresses, ports, protocol; the
    oracle over the rules without their residual fields finds it), so the frames in a MAC rule's box split into ones
    that hit it and ones that fall through to a later rule.  The corpus itself does not depend on the rules' MACs."""
    box = rules.copy()
    for f in ("smac", "dmac", "time_start", "time_end"):
        box[f] = 0
    ob = pyoracle.Oracle(box, default_action=1)
    first = ob.classify_batch(hdr, lens, cfg=ob.cfg(0, 1, NOW))["acl_hit"]
    seen = set()
    for k in np.nonzero(first >= 0)[0]:
        r = int(first[k])
        if r not in seen:
            seen.add(r)
            if rules["dmac"][r].any():
                rules["dmac"][r] = hdr[k, 0:6]
            if rules["smac"][r].any():
                rules["smac"][r] = hdr[k, 6:12]


_worlds = {}


def world(nrules):
    if nrules not in _worlds:
        _worlds[nrules] = World(nrules)
    return _worlds[nrules]


def to_device(hdr, lens, ts=None):
    """Device copies with PAST rows of 0xA5 behind the n real ones."""
    n, stride = hdr.shape
    th = torch.full((n + PAST, stride), 0xA5, dtype=torch.uint8, device=DEV)
    th[:n] = torch.from_numpy(np.ascontiguousarray(hdr)).to(DEV)
    tl = torch.full((n + PAST,), int(np.int32(-0x5A5A5A5B)), dtype=torch.int32, device=DEV)  # 0xA5A5A5A5
    tl[:n] = torch.from_numpy(np.ascontiguousarray(lens, np.uint32).view(np.int32)).to(DEV)
    tt = None
    if ts is not None:
        tt = torch.full((n + PAST,), 0x25A5A5A5A5A5A5A5, dtype=torch.int64, device=DEV)
        tt[:n] = torch.from_numpy(np.ascontiguousarray(ts, np.uint64).view(np.int64)).to(DEV)
    return th, tl, tt


FILL = {"part8": 0xEE}


def alloc_out(n, layout):
    """Output tensors of a layout, each with GUARD entries past what the engine may write."""
    shapes = {"tile_cnt": ((n + 63) // 64 + GUARD,), "tuple": (n + GUARD, 4)}
    names = {"soa": ("verdict", "flow_hash", "acl_hit", "fw_idx", "drop_idx", "tile_cnt", "tuple"),
             "part": ("verdict", "flow_hash", "acl_hit", "part_idx"),
             "part8": ("verdict", "flow_hash", "acl_hit", "part8"),
             "packed": ("packed", "part8")}[layout]
    out = {}
    for k in names:
        dt = torch.uint8 if k == "part8" else torch.int64 if k == "packed" else torch.int32
        out[k] = torch.full(shapes.get(k, (n + GUARD,)), FILL.get(k, -7), dtype=dt, device=DEV)
    return out


def result_ptrs(out):
    p = {k: v.data_ptr() for k, v in out.items()}
    if "part_idx" in p:  # partition layout: one list passed as both fw_idx and drop_idx
        p["fw_idx"] = p["drop_idx"] = p.pop("part_idx")
    return p


def collect(out, n, layout):
    """Host copies of the outputs as the checks read them; the guard entries must be untouched."""
    res = {}
    for k, v in out.items():
        a = v.cpu().numpy()
        m = (n + 63) // 64 if k == "tile_cnt" else n
        fill = np.array(FILL.get(k, -7)).astype(a.dtype)
        assert (a[m:] == fill).all(), f"{layout}: {k} written past its {m} entries"
        res[k] = a if k in ("acl_hit", "part8", "packed") else a.view(np.uint32)
    if layout == "packed":
        res.update(abi.unpack(res["packed"][:n]))
    for k in ("verdict", "flow_hash", "acl_hit", "tuple"):
        if k in res:
            res[k] = res[k][:n]
    return res


def check_lists(res, n, layout):
    if layout == "soa":
        check_compaction(res, n)
    elif layout == "part":
        check_partition(res, n)
    else:
        check_part8(res, n)


def classify(eng, dev, n, stride, layout, cfg):
    th, tl, tt = dev
    out = alloc_out(n, layout)
    eng.classify_ptrs(th.data_ptr(), tl.data_ptr(), n, stride, result_ptrs(out), cfg,
                      tt.data_ptr() if tt is not None else None, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return collect(out, n, layout)


def run_and_check(eng, w, stride, layout, syn=1, unsup=0, what=""):
    exp = w.expected(stride, syn, unsup)
    eng.clear_counters()
    res = classify(eng, w.device(stride), w.n, stride, layout, eng.cfg(unsup, syn, NOW))
    what = f"{what} stride {stride} {layout} syn_check {syn} unsupport_proto_action {unsup}:"
    dc.assert_matches(res, exp, w.meta, what,
                      keys=("verdict", "flow_hash", "acl_hit") + (("tuple",) * (layout == "soa")))
    check_lists(res, w.n, layout)
    got = dc.counters_list(eng.counters())
    assert got == exp["counters"].tolist(), (what, [(c, g, int(e)) for c, g, e in
                                                    zip(abi.COUNTERS, got, exp["counters"]) if g != int(e)])


@pytest.mark.parametrize("nrules", [256, 4096])
@pytest.mark.parametrize("tune,fam256,fam4096", TUNINGS, ids=[tune_id(t[0]) for t in TUNINGS])
def test_corpus_every_family_stride_layout(eng, nrules, tune, fam256, fam4096):
    w = world(nrules)
    eng.commit(w.rules, default_action=1)
    old = eng.tuning()
    try:
        eng.tuning(**tune)
        info = eng.launch_info()
        assert (info["fetch"], info["image"]) == (fam256 if nrules == 256 else fam4096), (tune, info)
        for stride in STRIDES:
            for layout in LAYOUTS:
                for syn in (1, 0):
                    run_and_check(eng, w, stride, layout, syn, what=f"{nrules} rules {tune_id(tune)}")
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("nrules", [256, 4096])
def test_corpus_unsupport_proto_action(eng, nrules):
    """ppe_cfg_t.unsupport_proto_action = 1 forwards what the decoders do not support (decode.c:33-36: L2_UNSUPPORT,
    VLAN_UNSUPPORT, IPV4_UNSUPPORT) instead of dropping it; no other status changes its action."""
    w = world(nrules)
    eng.commit(w.rules, default_action=1)
    e0, e1 = w.expected(128, 1, 0), w.expected(128, 1, 1)
    st, a0, a1 = e0["verdict"] & 0xFF, (e0["verdict"] >> 8) & 0xFF, (e1["verdict"] >> 8) & 0xFF
    unsup = np.isin(st, [abi.ST["L2_UNSUPPORT"], abi.ST["VLAN_UNSUPPORT"], abi.ST["IPV4_UNSUPPORT"]])
    for s in ("L2_UNSUPPORT", "VLAN_UNSUPPORT", "IPV4_UNSUPPORT"):
        assert (st == abi.ST[s]).any(), s
    assert (a0[unsup] == 1).all() and (a1[unsup] == 0).all() and np.array_equal(a0[~unsup], a1[~unsup])
    for stride in (64, 128):
        for layout in LAYOUTS:
            for unsup_action in (0, 1):
                run_and_check(eng, w, stride, layout, 1, unsup_action, what=f"{nrules} rules")


def tail_frames(w):
    """Three slow-path frames that reach the ACL: a TCP untagged one, a UDP tagged one, one that hits a rule."""
    e = w.expected(256)
    acl = (((e["verdict"] >> 16) & abi.F_ACL) != 0) & (w.meta["ihl"] > 5) & (np.arange(w.n) >= 64)
    a = np.nonzero(acl & (w.meta["proto"] == 6) & (w.meta["l2"] == "untagged"))[0][0]
    b = np.nonzero(acl & (w.meta["proto"] == 17) & (w.meta["l2"] != "untagged"))[0][0]
    c = np.nonzero(acl & (e["acl_hit"] >= 0) & ~np.isin(np.arange(w.n), [a, b]))[0][0]
    return int(a), int(b), int(c)


@pytest.mark.parametrize("nrules", [256, 4096])
@pytest.mark.parametrize("tune", [dict(), dict(pipeline=3), dict(pipeline=5)], ids=tune_id)
def test_batch_tails(eng, nrules, tune):
    """A batch whose last packet has IPv4 options: the lanes past the end of the batch carry that packet's window,
    and (multi-tile kernels) whole tiles of them are decoded.  The batch up to the frame, 65 packets with the frame
    alone in the last tile, and the frame alone, at a window where the slow path reads (128) and one where frames
    behind long options punt (64)."""
    w = world(nrules)
    eng.commit(w.rules, default_action=1)
    old = eng.tuning()
    try:
        eng.tuning(**tune)
        for j in tail_frames(w):
            for lo in (0, j - 64, j):
                sl = slice(lo, j + 1)
                n = j + 1 - lo
                for stride in (64, 128):
                    full = w.expected(stride)
                    exp = {k: v[sl] for k, v in full.items() if k != "counters"}
                    meta = {k: v[sl] for k, v in w.meta.items()}
                    dev = to_device(w.hdr[sl, :stride], w.lens[sl])
                    for layout in ("soa", "part"):
                        res = classify(eng, dev, n, stride, layout, eng.cfg(0, 1, NOW))
                        what = f"{nrules} rules {tune_id(tune)} frames [{lo}, {j}] stride {stride} {layout}:"
                        dc.assert_matches(res, exp, meta, what,
                                          keys=("verdict", "flow_hash", "acl_hit") + (("tuple",) * (layout == "soa")))
                        check_lists(res, n, layout)
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("tune", [dict(), dict(lds_image=0)], ids=tune_id)
def test_corpus_residual_rules(eng, tune):
    """Rules with MAC and time-window fields (their residual records re-read the frame's MACs from the window and its
    timestamp from batch.ts, both rare-path global reads) over slow-path and tagged frames."""
    w = world(300)
    if w.ts is None:
        w.ts = synth.make_packets(w.n, w.rules, seed=71, stride=128, with_ts=True)["ts"]
    eng.commit(w.rules, default_action=1)
    exp = w.expected(128)
    mac = w.rules["smac"].any(axis=1) | w.rules["dmac"].any(axis=1)
    tim = (w.rules["time_start"] != 0) | (w.rules["time_end"] != 0)
    hit = exp["acl_hit"]
    on_resid = (hit >= 0) & (mac | tim)[np.maximum(hit, 0)]
    assert on_resid.sum() >= 20, on_resid.sum()
    assert (on_resid & (w.meta["ihl"] > 5)).any() and (on_resid & (w.meta["l2"] != "untagged")).any()
    assert ((hit >= 0) & mac[np.maximum(hit, 0)]).sum() >= 10 and ((hit >= 0) & tim[np.maximum(hit, 0)]).sum() >= 10
    old = eng.tuning()
    try:
        eng.tuning(**tune)
        for layout in ("soa", "part"):
            run_and_check(eng, w, 128, layout, what=f"residual rules {tune_id(tune)}")
    finally:
        eng.tuning(**old)


RING_STRIDES = (64, 256, 80, 128, 96, 144)


@pytest.mark.parametrize("per_launch", ["0", "5"])
@pytest.mark.parametrize("nrules,tune", [(256, dict()), (4096, dict()), (4096, dict(pipeline=3))],
                         ids=["256-default", "4096-default", "4096-pipeline=3"])
def test_mixed_ring_calls(monkeypatch, nrules, tune, per_launch):
    """One ppe_classify_batches call over batches of different strides and sizes (12 descriptors, and 36: past the 32
    the kernel arguments hold), each batch a rolled slice of the corpus in its own buffer: the pipelined multi-tile
    loop prefetches the next descriptor's windows with that descriptor's n and stride, the cut-list kernel switches
    descriptors per wave."""
    monkeypatch.setenv("PPE_BATCHES_PER_LAUNCH", per_launch)
    w = world(nrules)
    eng = Engine(0)
    try:
        eng.commit(w.rules, default_action=1)
        eng.tuning(**tune)
        sizes = (w.n, 1, 65, 129, 257, w.n - 1)
        cfg = eng.cfg(0, 1, NOW)
        s = torch.cuda.current_stream(DEV)
        for K in (12, 36):
            bats, ress, keep = [], [], []
            for b in range(K):
                stride, n = RING_STRIDES[b % 6], sizes[b % 6]
                idx = np.roll(np.arange(w.n), -(131 * b + 7))[:n]
                dev = to_device(w.hdr[idx, :stride], w.lens[idx])
                out = alloc_out(n, "part")
                p = result_ptrs(out)
                bats.append(abi.Batch(dev[0].data_ptr(), dev[1].data_ptr(), None, n, stride))
                ress.append(abi.Result(p["verdict"], p["flow_hash"], p["acl_hit"], p["fw_idx"], p["drop_idx"], None,
                                       None))
                keep.append((dev, out, idx, stride, n))
            ins, outs = (abi.Batch * K)(*bats), (abi.Result * K)(*ress)
            eng.clear_counters()
            assert eng.lib.ppe_classify_batches(eng.ctx, ins, outs, K, C.byref(cfg), C.c_void_p(s.cuda_stream)) == 0
            torch.cuda.synchronize()
            total = np.zeros(32, np.uint64)
            fulls = {stride: w.expected(stride) for stride in RING_STRIDES}
            oracle = w.oracle
            for b, (dev, out, idx, stride, n) in enumerate(keep):
                res = collect(out, n, "part")
                full = fulls[stride]
                exp = {k: v[idx] for k, v in full.items() if k != "counters"}
                meta = {k: v[idx] for k, v in w.meta.items()}
                dc.assert_matches(res, exp, meta, f"{K} batches, batch {b} (n {n}, stride {stride}):",
                                  keys=("verdict", "flow_hash", "acl_hit"))
                check_partition(res, n)
                total += dc.expected_counters(oracle, w.hdr[idx], w.lens[idx], full["punt"][idx],
                                              (full["verdict"][idx] >> 16) & abi.F_VLAN != 0, oracle.cfg(0, 1, NOW))
            assert dc.counters_list(eng.counters()) == [int(x) for x in total]
    finally:
        eng.close()
