"""tests/flow_corpus.py on the CPU: pyoracle.OracleFlow (the C oracle's own hash table, pinned to flow.c by
test_oracle_flow.py) equals FlowModel (a dict, no table) on every step of every family and geometry, and the corpus
reaches the table layouts it aims at (LayoutSim).  What the GPU tests of test_gpu_flow_edges.py run is exactly this."""
from collections import Counter

import numpy as np
import pytest

import flow_corpus as fc
import pyoracle
from ppe import abi
from ppe.abi import ST

# cases per (family, geometry): a family that shrinks is noticed
COUNTS = {("run", "g64"): 30, ("run", "g1k"): 30, ("run", "g64k"): 30,
          ("displace", "g64"): 4, ("displace", "g1k"): 4, ("displace", "g64k"): 4,
          ("tomb", "g64"): 3, ("tomb", "g1k"): 3, ("tomb", "g64k"): 3, ("rehash", "g64"): 1,
          ("age", "g64"): 1, ("age", "g1k"): 1, ("age", "g64k"): 1,
          ("tuple", "g64"): 4, ("tuple", "g1k"): 4, ("tuple", "g64k"): 4,
          ("order", "g64"): 4, ("order", "g1k"): 5, ("order", "g64k"): 6,
          ("pool", "g64"): 4, ("pool", "g1k"): 4,
          ("update", "g1k"): 3, ("update", "g64k"): 3, ("update_hooks", "g1k"): 10, ("update_hooks", "g64k"): 10}


@pytest.fixture(scope="module")
def oracle():
    return pyoracle.Oracle(fc.rules(), default_action=fc.DROP)


_ran = {}


def ran(family, gname, oracle, pad=0):
    """Every case of a family through the model and the simulator, once per module."""
    k = (family, gname, pad)
    if k not in _ran:
        _ran[k] = [(c,) + fc.run_model(c, oracle) for c in fc.cases(family, gname, pad)]
    return _ran[k]


def test_family_sizes():
    assert set(fc.PAIRS) == set(COUNTS)
    got = {k: len(fc.cases(*k)) for k in fc.PAIRS}
    print(got)
    assert got == COUNTS


def test_key_search_is_quick_and_right():
    import time
    for g in (fc.G64, fc.G1K, fc.G64K, fc.BIG):
        t0 = time.perf_counter()
        for h in fc.homes(g):
            ks = fc.keys(g, h, 9)
            assert len(set(ks)) == 9 and all(fc.flow_hash(k) & g.gmask == h for k in ks)
            assert fc.flow_hash((ks[0][1], ks[0][0], ks[0][3], ks[0][2], ks[0][4])) == fc.flow_hash(ks[0])  # symmetric
        tcp = fc.keys(g, 5, 2, proto=6)
        assert all(fc.flow_hash(k) & g.gmask == 5 for k in tcp)
        print(g, f"{time.perf_counter() - t0:.3f} s")
    a = fc.keys(fc.G1K, 5, 1)[0]
    assert fc.flow_hash(a) != fc.flow_hash(a[:4] + (6,))   # the hash depends on the protocol


@pytest.mark.parametrize("family,gname", fc.PAIRS)
def test_oracle_equals_model(oracle, family, gname):
    """Verdict, acl_hit, flow_hash, counters, dump, stats and the aging return values, step by step."""
    for c, steps, _, _ in ran(family, gname, oracle):
        ft = pyoracle.OracleFlow(oracle, capacity=c["capacity"])
        try:
            for k, (s, m) in enumerate(zip(c["steps"], steps)):
                what = (c["name"], k, s.get("tag"))
                if s["kind"] == "batch":
                    ref = ft.classify_batch(s["hdr"], s["lens"], cfg=oracle.cfg(0, 1, s["now"]))
                    for f in ("verdict", "acl_hit", "flow_hash", "counters"):
                        assert np.array_equal(ref[f], m["res"][f]), (what, f)
                else:
                    assert ft.age(s["now"], s["timeout"]) == m["res"], what
                assert fc.dump_table(ft.dump()) == m["table"], what
                assert ft.stats() == m["stats"], what
        finally:
            ft.close()


@pytest.mark.parametrize("family,gname", fc.PAIRS)
def test_every_directed_packet_reaches_the_table(oracle, family, gname):
    """No case is exempt: every packet carries F_L4 (decoded to its ports) and none punts at the 64-byte window."""
    for c in fc.cases(family, gname):
        for s in c["steps"]:
            if s["kind"] == "batch":
                r = oracle.classify_batch(s["hdr"], s["lens"], cfg=oracle.cfg(0, 1, s["now"]))
                assert ((r["verdict"] >> 16) & abi.F_L4).all(), c["name"]
                assert ((r["verdict"] & 0xFF) != ST["WINDOW_PUNT"]).all() and (r["reach"] <= fc.STRIDE).all()


@pytest.mark.parametrize("gname", list(fc.GEOMS))
def test_layout_coverage(oracle, gname):
    seen = Counter()
    for family, g in fc.PAIRS:
        if g == gname:
            for _, _, _, sim in ran(family, g, oracle):
                seen.update(sim.seen)
    print(gname, dict(seen))
    need = ["full_group", "run_over_3_groups", "run_wraps", "live_behind_tomb", "claim_passes_tomb"]
    need += ["rehash_due"] if gname == "g64" else ["bucket_overflow"]
    need += ["owner_change_in_run"] if gname == "g1k" else []
    for k in need:
        assert seen[k] > 0, (gname, k)


def test_rehash_happens_and_keeps_every_keeper(oracle):
    (c, steps, m, sim), = ran("rehash", "g64", oracle)
    assert sim.rehashes >= 1 and steps[-1]["stats"]["live"] == 11
    assert all(r[5] + r[6] >= 6 and r[9] == fc.NOW + 701 for r in steps[-1]["table"])   # counters and last-seen


def test_aging_edges(oracle):
    for g in ("g64", "g1k", "g64k"):
        (_, _, m, _), = ran("age", g, oracle)
        want = {("T", False), ("T+1", True), ("now==L", False), ("now<L", False), ("now==L,T0", False), ("T0", True)}
        assert want <= set(m.age_cases), sorted(m.age_cases)
        assert not any(died for (kind, died) in m.age_cases if kind in ("T", "now==L", "now<L", "now==L,T0"))


def test_tomb_family(oracle):
    for g in ("g64", "g1k", "g64k"):
        for c, steps, _, sim in ran("tomb", g, oracle):
            assert sim.seen["live_behind_tomb"] and sim.seen["claim_passes_tomb"], c["name"]
            k = [i for i, s in enumerate(c["steps"]) if s.get("tag") == "new key; aged key again"][0]
            v = steps[k]["res"]["verdict"]
            # the new key; the aged key's reverse packet has no rule (DROP); its forward packet is a new flow again
            assert [int(x) & 0xFF for x in v[-3:]] == [0, ST["ACL_DROP"], 0]
            assert all((int(x) >> 16) & abi.F_NEWFLOW for x in (v[-3], v[-1]))
            assert steps[k]["tombs"] == 2


def test_order_creator_is_the_lowest_index(oracle):
    n = 0
    for g in ("g64", "g1k", "g64k"):
        for c, steps, _, _ in ran("order", g, oracle):
            if "creators" not in c["meta"]:
                continue
            ev, st = steps[0]["res"]["events"], steps[0]["res"]["stateless"]
            new = [(i, canon) for what, _, i, canon in ev if what == "new"]
            assert len(new) == 1 and new[0][0] == c["meta"]["creators"][0]
            others = [i for what, _, i, canon in ev if what == "found_new" and canon != new[0][1] and
                      int(st[i]) & 0xFF == ST["ACL_FW"]]
            assert others and min(others) > new[0][0]
            assert set(c["meta"]["creators"][1:]) <= set(others)
            if g == "g64k":   # different workgroups of the two-launch path
                assert len({i // fc.WG for i in c["meta"]["creators"]}) >= 2
            n += 1
    assert n == 5


def test_pool_grants_and_refusals(oracle):
    for g in ("g64", "g1k"):
        for c, steps, _, _ in ran("pool", g, oracle):
            k = [i for i, s in enumerate(c["steps"]) if s.get("tag") == "creators"][0]
            assert steps[k - 1]["stats"]["live"] == c["capacity"] - c["meta"]["free"]
            ev = steps[k]["res"]["events"]
            granted = [i for what, _, i, _ in ev if what == "new"]
            refused = [i for what, _, i, _ in ev if what == "nomem"]
            assert len(granted) == c["meta"]["free"]
            if c["meta"]["creators"] > c["meta"]["free"]:
                assert len(refused) >= 3 and min(refused) > max(granted)   # the creator and each of its repeats
                assert steps[k]["tombs"] == 1
            else:
                assert not refused and steps[k]["tombs"] == 0
            assert any(what == "found_new" for what, _, _, _ in ev)


def test_fold_edges_hit_the_thresholds(oracle):
    for g in ("g1k", "g64k"):
        (c, steps, _, _), = [r for r in ran("update_hooks", g, oracle) if r[0]["name"] == "fold-edges"]
        rows = steps[2]["table"]                  # after the second parts
        assert sorted(r[6] for r in rows) == [2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 4, 4]          # d2s packets
        assert sorted(r[8] for r in rows if r[8] > 300) == [499, 499, 500, 500, 501, 501]  # d2s bytes


def test_padded_form_is_the_same_traffic(oracle):
    """pad: the two-launch path's multi-workgroup form puts fillers in front of every batch and changes nothing else."""
    for family in ("order", "tomb"):
        for (c0, s0, _, _), (c1, s1, _, _) in zip(ran(family, "g64k", oracle), ran(family, "g64k", oracle, pad=768)):
            assert [x["table"] for x in s0] == [x["table"] for x in s1]
            assert all(len(s["lens"]) > 768 for s in c1["steps"] if s["kind"] == "batch")


def test_confusable_keys_lie_on_one_probe_path(oracle):
    """Keys in different home groups are never compared.  The port-swapped pair shares its home group; the UDP twin lies
    in the TCP twin's home group (behind the tombstones) when the SYN arrives, and both end up live."""
    for g in fc.GEOMS.values():
        a, b = fc.swap_ports_pair(g)
        assert fc.flow_hash(a) & g.gmask == fc.flow_hash(b) & g.gmask
        (c, steps, m, sim), = [r for r in ran("tuple", g.name, oracle) if r[0]["name"] == "tuple-protocol-twins"]
        u, t = c["meta"]["twins"]
        ku, kt = fc.flow_key(*u), fc.flow_key(*t)
        assert sim.find(ku) // 4 == sim.home(kt) and sim.find(kt) is not None and sim.home(ku) != sim.home(kt)
        assert steps[-1]["stats"]["live"] == 2
        k = [i for i, s in enumerate(c["steps"]) if s.get("tag") == "the TCP twin"][0]
        v = steps[k]["res"]["verdict"]
        assert int(v[0]) & 0xFF == ST["FLOW_TCP_NO_SYN_FIRST"] and (int(v[1]) >> 16) & abi.F_NEWFLOW
