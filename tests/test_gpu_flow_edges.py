"""The flow table's edges on the GPU: every step of tests/flow_corpus.py (full probe groups, runs that spill and wrap,
tombstones in front of live keys, contended claims, creators of one tuple in both orientations, pool overflow in packet
order, update buckets past 16 entries, fold and aging thresholds) through the engine, bit-exact against FlowModel (a
dict: no table, no probing) and, as a cross-check, against the oracle's own table: per-packet verdict, flow hash and ACL
hit, the compacted / partitioned lists, the counters, the dumped table, live / new_flow / del_flow and the tombstone count
after every step, and ppe_flow_age's return values.  flow_info()["slots"] is checked against the geometry the keys were
searched for: a corpus aimed at the wrong mask tests nothing.

Paths: the one-launch kernel and the two launches side by side (Trio), the two launches over several workgroups (768
fillers ahead of every batch), ppe_classify_flow_host with chunk boundaries inside the batches, a table of 2^24 slots
(8-byte global bucket entries), the kernel with the port-scan detector inside, and the post kernel with the monitors
flow-attached.  Integer work: no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (loads the HIP runtime first)

import flow_corpus as fc  # noqa: E402
from ppe import Engine, abi  # noqa: E402
from test_gpu_flow import Pair  # noqa: E402
from test_gpu_flow_small import CUTOFF, Trio  # noqa: E402

PAD = 768   # fillers ahead of every batch: a multiple of the 256-packet workgroup, past the one-launch cutoff


@pytest.fixture(scope="module")
def engines():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = (Engine(0), Engine(0))
    yield e
    for x in e:
        x.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines[0]


_model = {}


def modelled(family, gname, pad=0):
    """The family's cases with FlowModel's and LayoutSim's answers per step, computed once."""
    k = (family, gname, pad)
    if k not in _model:
        _model[k] = [(c, fc.run_model(c)[0]) for c in fc.cases(family, gname, pad)]
    return _model[k]


def same_packets(got, m, what):
    for k in ("verdict", "flow_hash", "acl_hit"):
        bad = np.flatnonzero(got[k] != m["res"][k])
        assert len(bad) == 0, (what, k, bad[:8].tolist(), got[k][bad[:4]].tolist(), m["res"][k][bad[:4]].tolist())


def same_table(e, geom, m, what):
    info = e.flow_info()
    assert info["slots"] == geom.nslots, (what, info)
    assert fc.dump_table(e.flow_dump()) == m["table"], what
    assert (info["live"], info["new_flow"], info["del_flow"]) == \
        (m["stats"]["live"], m["stats"]["new_flow"], m["stats"]["del_flow"]), (what, info)
    assert info["tombstones"] == m["tombs"], (what, info, m["tombs"])
    return info


def trio_case(engines, c, steps):
    t = Trio(engines, fc.rules(), capacity=c["capacity"], max_batch=c["geom"].max_batch, default_action=fc.DROP,
             env=c["env"])
    try:
        for k, (s, m) in enumerate(zip(c["steps"], steps)):
            what = f"{c['name']} step {k} {s.get('tag', 'age')}"
            if s["kind"] == "batch":
                ref = t.step(s["hdr"], s["lens"], s["now"], what=what)   # both engines == the oracle, lists, guards
                same_packets(ref, m, what)
            else:
                want = t.ft.age(s["now"], s["timeout"])
                assert [e.flow_age(s["now"], s["timeout"]) for e in (t.a, t.b)] == [want, want] and want == m["res"], what
                t.same()
            for e in (t.a, t.b):
                info = same_table(e, c["geom"], m, what)
        return info
    finally:
        t.close()


def pair_case(eng, c, steps, geom=None, launches=None, attach=None, verify=None, host_chunk=0):
    """One engine (test_gpu_flow.Pair: the engine and the oracle's table).  attach(eng) -> an attached object with
    close(); verify(obj): its own counters after every step; host_chunk: through ppe_classify_flow_host instead."""
    geom = geom or c["geom"]
    p = Pair(eng, fc.rules(), capacity=c["capacity"], max_batch=geom.max_batch, default_action=fc.DROP)
    obj = attach(eng) if attach else None
    try:
        for k, (s, m) in enumerate(zip(c["steps"], steps)):
            what = f"{c['name']} step {k} {s.get('tag', 'age')}"
            if s["kind"] == "batch" and host_chunk:
                got = eng.classify_flow_host(s["hdr"], s["lens"], cfg=eng.cfg(0, 1, s["now"]), chunk=host_chunk)
                ref = p.ft.classify_batch(s["hdr"], s["lens"], cfg=p.o.cfg(0, 1, s["now"]))
                same_packets(got, dict(res=ref), what + " (oracle)")
                same_packets(got, m, what)
                p.counters += ref["counters"]
                cnt = eng.counters()
                assert [cnt[x] for x in abi.COUNTERS] == p.counters[:len(abi.COUNTERS)].tolist(), what
            elif s["kind"] == "batch":
                got, _ = p.batch(s["hdr"], s["lens"], s["now"], part=(False, True, "8")[k % 3])
                same_packets(got, m, what)
                if launches:
                    assert eng.flow_launch_info() == launches(len(s["lens"])), what
            else:
                want = p.ft.age(s["now"], s["timeout"])
                assert eng.flow_age(s["now"], s["timeout"]) == want == m["res"], what
            p.same_table()
            info = same_table(eng, geom, m, what)
            if verify:
                verify(obj, what)
        return info
    finally:
        if obj is not None:
            obj.close()
        p.close()


# ---- the one-launch kernel and the two launches, side by side ----
@pytest.mark.parametrize("family,gname", fc.PAIRS)
def test_one_launch_and_two_launches(engines, family, gname):
    """engines[0] takes the one-launch kernel for every batch of at most the cutoff, engines[1]'s table was created
    under PPE_FLOW_SMALL=0 (Trio.step asserts which path each batch took); the update_hooks family's tables are created
    under PPE_FLOW_UPD_HASH / PPE_FLOW_FOLD_*."""
    assert CUTOFF >= 2 * fc.WG
    for c, steps in modelled(family, gname):
        info = trio_case(engines, c, steps)
        if family == "rehash":
            assert info["rehashes"] >= 1


@pytest.mark.parametrize("family", ["run", "displace", "tomb", "age", "tuple", "order", "update"])
def test_two_launches_over_several_workgroups(eng, family):
    """g64k with 768 fillers ahead of every batch: the directed packets lie in the classify launch's fourth and later
    workgroups, the order family's creators in different ones, finalize runs over more than one workgroup."""
    for c, steps in modelled(family, "g64k", PAD):
        pair_case(eng, c, steps, launches=lambda n: (0, 2))


def chunk_splits(c, chunk):
    """A run of 5 or more keys created in one batch, and the order family's creators: the batch is longer than a chunk."""
    if not (c["name"].startswith("run-batch") and c["meta"]["k"] >= 5) and "creators" not in c["meta"]:
        return True
    return max(len(s["lens"]) for s in c["steps"] if s.get("tag") in ("create", "creators")) > chunk


# ---- ppe_classify_flow_host: a chunk boundary inside the creation batch / between the creators ----
@pytest.mark.parametrize("family,gname,pad,chunk", [("run", "g1k", 60, 64), ("run", "g64k", 60, 64),
                                                    ("order", "g1k", 0, 64), ("order", "g64k", 0, 256)])
def test_host_path_chunks(eng, family, gname, pad, chunk):
    """Chunks are whole tiles, so 60 fillers ahead of a run's creation batch put the boundary at 64 between its keys;
    the order family's creators (5 / 100 / 200, 63 / 64 / 70, 5 / 300 / 700, 250 / 259 / 296) fall into different
    chunks as they are.  The batches are plain numpy arrays (not pinned), so they take the staged, chunked route."""
    for c, steps in modelled(family, gname, pad):
        assert chunk_splits(c, chunk)
        pair_case(eng, c, steps, host_chunk=chunk)


# ---- more than 2^23 slots: 8-byte bucket entries in global memory ----
def test_table_of_2_to_the_24_slots(eng):
    """test_gpu_flow.py::test_flow_large_table_global_buckets' geometry with keys searched for its 2^22-group mask: runs
    of 9 from group 0 and from the last group (wrapping), one key per batch from a middle group, and the update family,
    all on one table (dumping 2^24 slots after every step would take minutes: per-packet outputs, counters, stats and
    tombstones after every step, the table once at the end)."""
    g = fc.BIG
    runs = {c["name"]: c for c in fc.fam_run(g)}
    h = fc.homes(g)
    picked = [runs[f"run-batch-h{h[0]}-k9"], runs[f"run-serial-h{h[1]}"], runs[f"run-batch-h{h[2]}-k9"]] + fc.fam_update(g)
    c = fc.case("big", g, [s for x in picked for s in x["steps"]])
    steps, _, sim = fc.run_model(c)
    assert sim.seen["run_wraps"] and sim.seen["run_over_3_groups"] and sim.seen["bucket_overflow"]
    p = Pair(eng, fc.rules(), capacity=g.capacity, max_batch=g.max_batch, default_action=fc.DROP)
    try:
        for k, (s, m) in enumerate(zip(c["steps"], steps)):
            got, _ = p.batch(s["hdr"], s["lens"], s["now"], part=(False, True, "8")[k % 3])
            same_packets(got, m, f"big step {k} {s['tag']}")
            info = eng.flow_info()
            assert (info["slots"], info["live"], info["tombstones"]) == (g.nslots, m["stats"]["live"], 0)
        p.same_table()
        same_table(eng, g, steps[-1], "big, at the end")
    finally:
        p.close()


# ---- the kernel with the port-scan detector inside (its own finalize) ----
VARIANT = [(f, g) for f in ("run", "tomb", "order", "pool") for g in fc.FAMILIES[f][1]]


@pytest.mark.parametrize("family,gname", VARIANT)
def test_with_the_port_scan_detector_inside(eng, family, gname):
    """A port-scan table flow-attached and enabled, its threshold one that no source reaches: the detector answers OK
    every time (its counters say so), so the flow table's answers are FlowModel's."""
    def attach(e):
        ps = e.portscan(attach="flow", able=1, action=0, exception_freq=1 << 30, hold_seconds=600, capacity=1 << 14,
                        max_batch=1024, cycles_per_second=1000)
        ps.clock(10_000, fc.NOW)
        return ps

    def verify(ps, what):
        i = ps.info()
        assert i["ok"] > 0 and (i["nomem"], i["detected"], i["hold"], i["drop"]) == (0, 0, 0, 0), (what, i)

    ran = 0
    for c, steps in modelled(family, gname):
        if max(len(s["lens"]) for s in c["steps"] if s["kind"] == "batch") > eng.flow_portscan_max():
            continue   # (the order family's 4,096-packet case: this kernel takes one workgroup's worth)
        pair_case(eng, c, steps, launches=lambda n: (2, 1), attach=attach, verify=verify)
        ran += 1
    assert ran >= len(modelled(family, gname)) - 1


# ---- the post kernel with the monitors flow-attached ----
@pytest.mark.parametrize("family,gname,pad", [(f, g, 0) for f, g in VARIANT] +
                         [(f, "g64k", PAD) for f in ("run", "tomb", "order")])
def test_with_monitors_flow_attached(eng, family, gname, pad):
    """Monitors flow-attached with no protection rule loaded: nothing is dropped (the drop totals stay 0), every batch
    takes the two launches (ppe_flow_post_attack_kernel), and the flow table's answers are FlowModel's."""
    def attach(e):
        a = e.attack(None, attach="flow")
        a.clock(fc.NOW)
        return a

    def verify(a, what):
        i = a.info()
        assert all(i[k] == 0 for k in abi.ATTACK_TOTALS), (what, i)

    for c, steps in modelled(family, gname, pad):
        pair_case(eng, c, steps, launches=lambda n: (0, 2), attach=attach, verify=verify)
