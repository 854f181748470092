"""The ACL rule-edge corpus (tests/acl_corpus.py) through every kernel that matches a key against the classifier
image: the stateless classify path in every fetch family and image placement (the node walk and rule records, the
2-level block walk and compact records, the cut lists), the StreamTcp instantiation, the flow-table path (two
launches, the one-launch small kernel, the host entry) and the tuple lookup on both sides of its global / LDS switch.

Bar: bit-exact against acl_corpus.linear, a numpy first match over the rule table that uses neither the oracle nor the
image: the hit index, and the verdict word derived from the matched action (only action 1 drops: ACL_DROP / ACL_FW,
the frame's own flags); the acl_fw / acl_drop counters exactly; the 64 guard entries past n of every output untouched.
A failure names the corpus cases it lost (the labels say which edge of which rule or node a key aims at).  The port-scan
and attack instantiations are not run here: a corpus with many ports per source trips the detector, and their models
have suites of their own."""
import ctypes as C
import re
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

from ppe import Engine, abi  # noqa: E402

import acl_corpus as ac  # noqa: E402
import test_gpu_decode_edges as de  # noqa: E402
from test_gpu_decode_edges import (DEV, alloc_out, check_lists, classify, collect, result_ptrs,  # noqa: E402
                                   to_device, tune_id)

NOW = ac.NOW
assert [t for t, _, _ in de.TUNINGS] == ac.TUNINGS  # every row of the decode sweep's table
assert [(a, b) for _, a, b in de.TUNINGS] == list(zip(ac.FAMILIES["r256"], ac.FAMILIES["r4096"]))


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = Engine(0)
    yield e
    e.close()


class World:
    """One rule set's frames, their device copies per stride and the expected answers, each made once."""

    def __init__(self, name):
        self.c = ac.corpus(name)
        self.hdr, self.lens, self.vlan, self.idx = self.c.frames(128)
        self.n = len(self.idx)
        self.tcp = self.c.keys["proto"][self.idx] == 6
        self.labels = self.c.labels[self.idx]
        self._dev = {}

    def commit(self, eng):
        eng.commit(self.c.rules, self.c.used, default_action=1)

    def device(self, stride, ts=False):
        if (stride, ts) not in self._dev:
            self._dev[stride, ts] = to_device(self.hdr[:, :stride], self.lens, self.c.ts[self.idx] if ts else None)
        return self._dev[stride, ts]

    def expected(self, now=None, flow=False, sel=slice(None)):
        """now None: every key at its own timestamp; else all of them at `now`."""
        hit, act = self.c.linear(ts=now, sel=self.idx)
        return dict(acl_hit=hit[sel], action=act[sel],
                    verdict=ac.expected(hit[sel], act[sel], self.tcp[sel], self.vlan[sel], flow))


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


def cases(labels):
    """The corpus cases behind a set of keys: their labels with the rule / node / cluster numbers and the corner and
    protocol suffixes taken out, most frequent first."""
    short = Counter(re.sub(r"^([rnc]|aim)\d+", r"\1", x).split("/")[0] for x in labels)
    return ", ".join(f"{k} x{v}" for k, v in short.most_common(16))


def check(res, exp, labels, what, counters=None, keys=("acl_hit", "verdict")):
    for k in keys:
        bad = np.flatnonzero(res[k] != exp[k])
        assert len(bad) == 0, (f"{what}: {k} wrong for {len(bad)} of {len(labels)} keys; cases: {cases(labels[bad])}; "
                               f"first (label, got, expected): "
                               f"{[(labels[b], int(res[k][b]), int(exp[k][b])) for b in bad[:4]]}")
    if counters is not None:
        check_counters(counters, exp, what)


def check_counters(counters, exp, what):
    n = len(exp["action"])
    drop = int((exp["action"] == abi.ACL_RULE_ACTION_DROP).sum())
    assert (counters["acl_drop"], counters["acl_fw"], counters["pkts"]) == (drop, n - drop, n), what


def run(eng, w, stride, layout, what, ts=False, now=NOW):
    exp = w.expected(None if ts else now)
    eng.clear_counters()
    res = classify(eng, w.device(stride, ts), w.n, stride, layout, eng.cfg(0, 1, now))
    what = f"{w.c.name} {what} stride {stride} {layout}"
    check(res, exp, w.labels, what, eng.counters())
    check_lists(res, w.n, layout)
    if layout == "soa":
        assert np.array_equal(res["tuple"][:, :3], ac.tuples(w.c.keys[w.idx])[:, :3]), what


def sweep(eng, w, what):
    for stride in (64, 128):
        for layout in ("soa", "packed"):
            run(eng, w, stride, layout, what)


@pytest.mark.parametrize("name", list(ac.FAMILIES))
@pytest.mark.parametrize("row", range(len(ac.TUNINGS)), ids=[tune_id(t) for t in ac.TUNINGS])
def test_stateless_every_family(eng, name, row):
    """acl_walk + rule_box (none / hoist), acl_walk_blocks_mt + crec_check (multi), acl_cut (cut), each with the image
    in LDS, split and in global memory; leaflist's 600-candidate leaf with its escaped count and MAC records."""
    w, tune = world(name), ac.TUNINGS[row]
    w.commit(eng)
    old = eng.tuning()
    try:
        eng.tuning(**tune)
        info = eng.launch_info()
        assert (info["fetch"], info["image"]) == ac.FAMILIES[name][row], (name, tune, info)
        sweep(eng, w, tune_id(tune))
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("lds_image", [1, 0])
@pytest.mark.parametrize("lines", ["0", "1"])
@pytest.mark.parametrize("bits", ["11", "16"])
def test_fifteen_cut_lists(eng, monkeypatch, bits, lines, lds_image):
    """Bucket lists of the maximum length 15 (a match at every position, none on either side), dense entries with
    their id array and 7-entry lines with the ids inside, entries in LDS and read from global memory."""
    monkeypatch.setenv("PPE_CUT_BITS", bits)
    monkeypatch.setenv("PPE_CUT_LINES", lines)
    w = world("fifteen")
    w.commit(eng)
    old = eng.tuning()
    try:
        eng.tuning(pipeline=5, lds_image=lds_image)
        info = eng.launch_info()
        assert (info["fetch"], info["image"]) == ("cut", "global" if not lds_image else "split" if lines == "1" else "lds")
        sweep(eng, w, f"{bits} bits lines {lines} lds_image {lds_image}")
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("tune", [dict(), dict(lds_image=0)], ids=tune_id)
def test_residual_rules(eng, tune):
    """resid_match: each MAC byte (both image words of a MAC), the time window's two ends with the packet's own
    timestamp and with the batch-wide now, windows that straddle 2^32."""
    w = world("resid")
    w.commit(eng)
    nows = [NOW, 2**32 - 2, ac.TIMEWRAP[0], 2**32, ac.TIMEWRAP[1], 2**32 + 2]
    r = w.c.rules
    timed = np.flatnonzero((r["time_start"] != 0) & (r["time_start"] < 2**32 - 1))[:2]
    for t in timed:
        nows += [int(r["time_start"][t]) - 1, int(r["time_start"][t]), int(r["time_end"][t]), int(r["time_end"][t]) + 1]
    old = eng.tuning()
    try:
        eng.tuning(**tune)
        for layout in ("soa", "packed"):
            run(eng, w, 128, layout, f"{tune_id(tune)} per-packet ts", ts=True)
        run(eng, w, 64, "soa", f"{tune_id(tune)} per-packet ts", ts=True)
        for now in nows:
            exp = w.expected(now)
            eng.clear_counters()
            res = classify(eng, w.device(128), w.n, 128, "soa", eng.cfg(0, 1, now))
            check(res, exp, w.labels, f"resid {tune_id(tune)} now {now}", eng.counters())
    finally:
        eng.tuning(**old)


def test_65536_rules(eng):
    """The sampled rule edges of the 65,536-rule set: the cut lists read from L2 (default), and the block walk."""
    w = world("r65536")
    w.commit(eng)
    old = eng.tuning()
    try:
        for tune, fam in ((dict(), ("cut", "split")), (dict(pipeline=3), ("multi", "split"))):
            eng.tuning(**tune)
            info = eng.launch_info()
            assert (info["fetch"], info["image"]) == fam, (tune, info)
            run(eng, w, 64, "soa", tune_id(tune))
            run(eng, w, 128, "packed", tune_id(tune))
    finally:
        eng.tuning(**old)


@pytest.mark.parametrize("name", ["r256", "r4096"])
def test_stream_tcp_instantiation(eng, name):
    """With StreamTcp's first-packet verdict on, a bare SYN forwards like before: the same answers from the STM
    kernels (node walk, block walk and cut lists)."""
    w = world(name)
    w.commit(eng)
    old = eng.tuning()
    try:
        assert eng.stream_tcp(track=1)["track"] == 1
        for tune in (dict(), dict(pipeline=1), dict(pipeline=3), dict(pipeline=5, lds_image=0)):
            eng.tuning(**tune)
            run(eng, w, 64, "soa", f"stream {tune_id(tune)}")
            run(eng, w, 128, "packed", f"stream {tune_id(tune)}")
    finally:
        eng.stream_tcp(track=0)
        eng.tuning(**old)


def classify_flow(eng, dev, n, stride, cfg):
    th, tl, _ = dev
    out = alloc_out(n, "soa")
    p = result_ptrs(out)
    b = abi.Batch(th.data_ptr(), tl.data_ptr(), None, n, stride)
    r = abi.Result(p["verdict"], p["flow_hash"], p["acl_hit"], p["fw_idx"], p["drop_idx"], p["tile_cnt"], p["tuple"],
                   None, None)
    eng._check(eng.lib.ppe_classify_flow(eng.ctx, C.byref(b), C.byref(r), C.byref(cfg),
                                         C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)), "ppe_classify_flow")
    torch.cuda.synchronize()
    return collect(out, n, "soa")


@pytest.mark.parametrize("name", ["r256", "r4096"])
def test_flow_table_path(eng, name):
    """One frame per flow, so every frame is a miss that walks the ACL in the FLOW kernels (4,096 rules: the one-tile
    split plan, whose walk crosses from the LDS levels to the global ones): one batch in two launches, slices of at
    most 512 through the one-launch kernel, and the host entry; a fresh table each time."""
    w = world(name)
    w.commit(eng)
    u = ac.flow_unique(w.c.keys[w.idx])
    n = len(u)
    exp = w.expected(flow=True, sel=u)
    labels, hdr, lens = w.labels[u], w.hdr[u], w.lens[u]
    cfg = eng.cfg(0, 1, NOW)
    try:
        eng.flow_create(n + 64, n)
        eng.clear_counters()
        res = classify_flow(eng, to_device(hdr[:, :64], lens), n, 64, cfg)
        assert eng.flow_launch_info() == (0, 2)
        check(res, exp, labels, f"{name} flow batch", eng.counters())
        assert eng.flow_info()["live"] == int((exp["action"] != 1).sum())
        eng.flow_destroy()
        eng.flow_create(n + 64, n)
        eng.clear_counters()
        a, k = 0, 0
        while a < n:
            m = min((512, 257, 64, 1, 511)[k % 5], n - a)
            sl = slice(a, a + m)
            res = classify_flow(eng, to_device(hdr[sl, :128], lens[sl]), m, 128, cfg)
            assert eng.flow_launch_info() == (1, 1)
            check(res, {x: v[sl] for x, v in exp.items()}, labels[sl], f"{name} flow slice [{a}, {a + m})")
            a, k = a + m, k + 1
        check_counters(eng.counters(), exp, f"{name} flow slices")
        eng.flow_destroy()
        eng.flow_create(n + 64, n)
        eng.clear_counters()
        res = eng.classify_flow_host(hdr[:, :64], lens, cfg=cfg, chunk=4096,
                                     outputs=("verdict", "flow_hash", "acl_hit"))
        check(res, exp, labels, f"{name} flow host", eng.counters())
    finally:
        eng.flow_destroy()


@pytest.mark.parametrize("name", ac.SETS)
def test_acl_lookup_host(eng, name):
    """The tuple kernel (acl_walk + rule_box + resid_match over pre-decoded tuples): every key of the corpus, the
    protocol edges and residual edges no frame carries among them, with their MACs and timestamps; whole (4,096-tuple
    chunks: the image staged in LDS where it fits) and in calls of 4,095 (read from global memory), and 1, 64, 4,096."""
    c = ac.corpus(name)
    eng.commit(c.rules, c.used, default_action=1)
    hit, act = c.linear()
    t, m = ac.tuples(c.keys), ac.mac_words(c.macs)

    def lookup(sl, what):
        h, a = eng.acl_lookup_host(t[sl], m[sl], c.ts[sl], now_seconds=NOW)
        check(dict(acl_hit=h, action=a), dict(acl_hit=hit[sl], action=act[sl]), c.labels[sl], f"{name} lookup {what}",
              keys=("acl_hit", "action"))

    lookup(slice(None), "whole")
    for a in range(0, c.n, 4095):
        lookup(slice(a, a + 4095), f"[{a}, +4095)")
    for size in (1, 64, 4096):
        lookup(slice(max(0, c.n - size), c.n), f"last {size}")
    if name == "resid":  # without per-tuple timestamps: the batch-wide now, on both sides of a window across 2^32
        for now in (ac.TIMEWRAP[0] - 1, ac.TIMEWRAP[0], ac.TIMEWRAP[1], ac.TIMEWRAP[1] + 1):
            h, a = eng.acl_lookup_host(t, m, None, now_seconds=now)
            eh, ea = c.linear(ts=now)
            check(dict(acl_hit=h, action=a), dict(acl_hit=eh, action=ea), c.labels, f"resid lookup now {now}",
                  keys=("acl_hit", "action"))
