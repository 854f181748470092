"""The promises of the ACL rule-edge corpus (tests/acl_corpus.py), on the CPU: its frames carry the keys they were
built from; the oracle's four walkers (the linear scan, the node tree, the 2-level blocks, the cut lists) equal the
numpy first match `linear` on every key, for hit, action and the whole verdict word, with default FW and DROP; and
the coverage conditions that make the corpus worth running on the GPU hold.  They are conditions on the built images,
asserted, not measurements: every internal node is entered with key == threshold and with key == threshold + 1; the
`fifteen` set's cut lists are matched at every position, entry slot and id half-word; the `leaflist` count is
escaped; every rule of `extremes` that can be a first match is one, next to a key that is not."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from ppe import abi

import acl_corpus as ac
from test_acl_build import cut_entries, cut_header, cut_lengths

NOW = ac.NOW
SMALL = [s for s in ac.SETS if s != "r65536"]


def oracle_of(c, default_action=1, img=None):
    img = c.img if img is None and default_action == 1 else img
    if img is None:
        img = abi.build_image(c.rules, c.used, default_action)[0]
    return pyoracle.Oracle(c.rules, c.used, default_action=default_action, image=img), img


def per_key(o, fn, c, sel):
    """One of the oracle's per-tuple walkers over keys[sel], with their MACs and timestamps."""
    f = getattr(o.lib, fn)
    hit, act = np.zeros(len(sel), np.int32), np.zeros(len(sel), np.uint32)
    a = C.c_uint32()
    for j, i in enumerate(sel):
        k, m = c.keys[i], c.macs[i]
        hit[j] = f(int(k["sip"]), int(k["dip"]), int(k["sport"]), int(k["dport"]), int(k["proto"]),
                   m[0:6].ctypes.data, m[6:12].ctypes.data, int(c.ts[i]), C.byref(a))
        act[j] = a.value
    return hit, act


def test_frames_carry_their_keys():
    """The decoder's tuple of every frame is the key it was built from; one frame in four is tagged, TCP frames are
    bare SYNs, and every frame reaches the ACL."""
    c = ac.corpus("extremes")
    hdr, lens, vlan, idx = c.frames()
    o, _ = oracle_of(c)
    r = o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW))
    k = c.keys[idx]
    assert np.array_equal(r["tuple"][:, :3], ac.tuples(k)[:, :3])
    assert np.array_equal(r["tuple"][:, 3] & 0x1FF, k["proto"].astype(np.uint32) | vlan.astype(np.uint32) << 8)
    fl = r["verdict"] >> 16
    assert ((fl & abi.F_ACL) != 0).all() and np.array_equal((fl & abi.F_VLAN) != 0, vlan)
    assert np.array_equal((fl & abi.F_SYN) != 0, k["proto"] == 6) and vlan.sum() == len(idx) // 4
    assert np.array_equal(hdr[:, 0:12], c.macs[idx])


@pytest.mark.parametrize("name,default_action", [(s, da) for s in ac.SETS for da in (1, 0)
                                                 if (s, da) != ("r65536", 0)])  # (one build of that image is enough)
def test_walkers_equal_linear(name, default_action):
    c = ac.corpus(name)
    o, img = oracle_of(c, default_action)
    hit, act = c.linear(default_action)
    hdr, lens, vlan, idx = c.frames()
    exp = ac.expected(hit[idx], act[idx], c.keys["proto"][idx] == 6, vlan)
    for walker in (False, True, 2) + ((3,) if img[22] else ()):
        r = o.classify_batch(hdr, lens, ts=c.ts[idx], cfg=o.cfg(0, 1, NOW), nthreads=8, use_tree=walker)
        bad = np.flatnonzero((r["acl_hit"] != hit[idx]) | (r["verdict"] != exp))
        assert len(bad) == 0, (walker, [(c.labels[idx[b]], int(r["acl_hit"][b]), int(hit[idx[b]])) for b in bad[:5]])
        assert int(r["counters"][abi.COUNTERS.index("acl_drop")]) == int((act[idx] == 1).sum())
        assert int(r["counters"][abi.COUNTERS.index("acl_fw")]) == int((act[idx] != 1).sum())
    # the keys no frame carries (other protocols), and a sample of the rest, through the per-tuple entry points
    sel = np.flatnonzero(~c.frame | (np.arange(c.n) % (64 if name == "r65536" else 8) == 0))
    for fn in ("oracle_acl_linear", "oracle_acl_tree"):
        h, a = per_key(o, fn, c, sel)
        bad = np.flatnonzero((h != hit[sel]) | (a != act[sel]))
        assert len(bad) == 0, (fn, [(c.labels[sel[b]], int(h[b]), int(hit[sel[b]])) for b in bad[:5]])


@pytest.mark.parametrize("name", SMALL)
def test_every_node_entered_on_both_sides(name):
    """Per internal node of the image, a key arrives equal to its threshold (goes left) and one equal to threshold + 1
    (goes right); no node is exempt in these images (its threshold inside its path's interval).  The frames alone do
    the same for every node a frame can reach on both sides."""
    c = ac.corpus(name)
    at, past, inner = ac.node_coverage(c.img, c.keys)
    assert len(c.exempt) == 0
    assert (at & past)[inner].all(), np.flatnonzero(inner & ~(at & past))[:10]
    at, past, _ = ac.node_coverage(c.img, c.keys[c.frame])
    assert (at & past)[c.by_frame].all() and 2 * len(c.by_frame) >= inner.sum()
    # the walk's fixed point: a key of 0xffffffff arrives at a leaf, whose threshold word it equals
    if name == "extremes":
        assert (c.keys["sip"][c.frame] == 0xFFFFFFFF).any() and (c.keys["dip"][c.frame] == 0xFFFFFFFF).any()


def buckets(h, keys):
    return (keys["sip"].astype(np.int64) >> (32 - h["b0"])) << h["b1"] | keys["dip"].astype(np.int64) >> (32 - h["b1"])


@pytest.mark.parametrize("lines", ["0", "1"])
@pytest.mark.parametrize("bits", ["11", "16"])
def test_fifteen_fills_the_cut_lists(monkeypatch, bits, lines):
    """`fifteen` under a forced cut: the oracle's cut walk equals `linear`; at 11 bits the eight clusters are eight
    lists of 15 whose first entries start at every phase of the 8-entry fingerprint word, every list position, entry
    slot and id half-word holds a match, and the node forest (so the corpus) is the one built without the variables."""
    c = ac.corpus("fifteen")
    monkeypatch.setenv("PPE_CUT_BITS", bits)
    monkeypatch.setenv("PPE_CUT_LINES", lines)
    img = abi.build_image(c.rules, None, 1)[0]
    assert int(img[22]) != 0
    nn = int(img[2])
    assert nn == int(c.img[2]) and np.array_equal(img[int(img[5]):int(img[5]) + 4 * nn],
                                                  c.img[int(c.img[5]):int(c.img[5]) + 4 * nn])
    o, _ = oracle_of(c, img=img)
    hit, act = c.linear()
    hdr, lens, vlan, idx = c.frames()
    r = o.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW), nthreads=8, use_tree=3)
    assert np.array_equal(r["acl_hit"], hit[idx])
    assert np.array_equal(r["verdict"], ac.expected(hit[idx], act[idx], c.keys["proto"][idx] == 6, vlan))
    h = cut_header(img)
    assert h["b0"] + h["b1"] == int(bits) and h["lines_ids"] == (lines == "1") and h["ids16"]
    if bits != "11":
        return
    assert (h["b0"], h["b1"]) == (3, 8) and h["max_len"] == 15
    lens_, (ent, ids) = cut_lengths(img, h), cut_entries(img, h)
    first = np.concatenate([[0], np.cumsum(lens_)])[:-1]
    full = np.flatnonzero(lens_ == 15)
    assert len(full) == ac.FIFTEEN_CLUSTERS and set(first[full] & 7) == set(range(8))
    k = c.keys[idx]
    bk = buckets(h, k)
    matched = np.flatnonzero((hit[idx] >= 0) & np.isin(bk, full))
    pos = np.array([int(np.flatnonzero(ids[first[b]:first[b] + lens_[b]] == x)[0])
                    for b, x in zip(bk[matched], hit[idx][matched])])
    e = first[bk[matched]] + pos
    assert set(pos) == set(range(15)) and set(e % h["epl"]) == set(range(h["epl"]))
    assert set((e % h["epl"] if h["lines_ids"] else e) & 1) == {0, 1}  # the id's 16-bit half of its word
    for cl in range(ac.FIFTEEN_CLUSTERS):  # both neighbours of every list miss
        for dport in (999, 1000 + ac.FIFTEEN_LEN):
            sel = np.array([x.startswith(f"c{cl}.dport{dport}/") for x in c.labels[idx]])
            assert sel.sum() == 2 and (hit[idx][sel] == -1).all() and (act[idx][sel] == 1).all()


def test_first_and_last_bucket_of_a_group_are_hit():
    """The popcount prefix of a group's length slices runs over k = bucket mod 32 lower buckets: matches fall into
    buckets with k == 0 (an empty mask) and k == 31 (the widest) in the images that have cut lists."""
    seen = set()
    for name in SMALL:
        c = ac.corpus(name)
        if not c.img[22]:
            continue
        hit, _ = c.linear()
        k = buckets(cut_header(c.img), c.keys[c.frame & (hit >= 0)]) & 31
        seen |= set(k[(k == 0) | (k == 31)])
    assert seen == {0, 31}


def test_leaflist_count_is_escaped():
    c = ac.corpus("leaflist")
    img = c.img
    nodes = img[img[5]:img[5] + 4 * img[2]].reshape(-1, 4)
    assert ((nodes[nodes[:, 0] == 0xFFFFFFFF][:, 2] >> 24) == 255).any() and img[12] >= ac.LEAFLIST_N
    hit, _ = c.linear()
    aimed = np.array([x.startswith("aim") for x in c.labels])
    assert {int(x) for x in hit[aimed]} == {-1, 0, 253, 254, 255, 599}  # (a flipped MAC bit may name another rule)


def test_every_rule_of_extremes_is_hit_and_missed():
    """Every rule that can be a first match (used, a non-empty box, not a lower-priority copy of an earlier box) is the
    first match of a key, and a key one step away in one field is not its match.  The others never are."""
    c = ac.corpus("extremes")
    hit, act = c.linear()
    never = set(np.flatnonzero(c.used == 0)) | set(c.shadowed) | set(c.empty)
    assert not never & set(hit)
    rule_of = np.array([int(lbl[1:lbl.index(".")]) if lbl[0] == "r" else -1 for lbl in c.labels])
    for r in sorted(set(range(len(c.rules))) - never):
        own = rule_of == r
        assert (hit[own] == r).any() and (hit[own] != r).any(), r
    # a frame finds each rule a frame can match: one whose protocol range holds 6 or 17 (but rule 8, which repeats
    # rule 7's box for the protocols outside 6-17)
    lo, hi = c.rules["protocol_start"], c.rules["protocol_end"]
    for r in sorted(set(np.flatnonzero(((lo <= 6) & (hi >= 6)) | ((lo <= 17) & (hi >= 17)))) - never - {8}):
        assert (hit[c.frame] == r).any(), r
    assert set(act[hit >= 0]) == {0, 1, 2, 0xFFFF}


def test_residual_edges_hit_and_miss():
    """MAC rules are matched by their own MACs and by none of the one-bit variants of the MAC they fix (each of the six
    bytes, so both image words of a MAC); time rules at start and end and not one second outside, the windows across
    2^32 among them."""
    c = ac.corpus("resid")
    hit, _ = c.linear()
    lab = c.labels
    rule_of = np.array([int(x[1:x.index(".")]) if x[0] == "r" else -1 for x in lab])
    kinds = set()
    for i in np.flatnonzero([x.endswith(".mac.own") for x in lab]):
        r = rule_of[i]
        if hit[i] != r:
            continue
        for which in ("dmac", "smac"):
            if c.rules[which][r].any():
                var = np.flatnonzero([x.startswith(f"r{r}.{which}.byte") for x in lab])
                assert len(var) == 6 and (hit[var] != r).all(), (r, which)
                kinds.add(which)
    assert kinds == {"dmac", "smac"}
    n_time = 0
    for r in np.flatnonzero((c.rules["time_start"] != 0) | (c.rules["time_end"] != 0)):
        at = {x.split(".")[-1]: i for i, x in enumerate(lab) if x.startswith(f"r{r}.time.")}
        if hit[at["start"]] == r:
            n_time += 1
            assert hit[at["end"]] == r and hit[at["end+1"]] != r and hit[at.get("start-1", at["end+1"])] != r, r
    assert n_time >= 20
    wrap = np.flatnonzero(c.rules["time_start"] == ac.TIMEWRAP[0])
    assert len(wrap) >= 2 and all(hit[[i for i, x in enumerate(lab) if x == f"r{r}.time.end"][0]] == r for r in wrap)


def test_planned_families():
    """The (fetch, image placement) table the GPU sweep asserts through ppe_launch_info is what the host-only planner
    decides for these images; the flow-table plan of the 4,096-rule image is the one-tile split walk (its top levels
    in LDS, the rest read from global memory)."""
    from test_launch_plan import plan_image
    for name, rows in ac.FAMILIES.items():
        img = ac.corpus(name).img
        for tune, fam in zip(ac.TUNINGS, rows):
            p = plan_image(img, tune, 0)
            assert (ac.PLAN_FETCH[p["pipe"]], ac.PLAN_IMAGE[p["mode"]]) == fam, (name, tune)
    assert {f for rows in ac.FAMILIES.values() for f, _ in rows} == {"hoist", "none", "multi", "cut"}
    p = plan_image(ac.corpus("r4096").img, {}, 1)
    assert (ac.PLAN_FETCH[p["pipe"]], ac.PLAN_IMAGE[p["mode"]]) == ("hoist", "split") and 0 < p["lds_iters"] <= p["max_depth"]


def test_flow_unique_keeps_one_key_per_flow():
    c = ac.corpus("r256")
    idx = np.flatnonzero(c.frame)
    u = idx[ac.flow_unique(c.keys[idx])]
    k = c.keys[u]
    fwd = {(int(a), int(b), int(p), int(q), int(t)) for a, b, p, q, t in k.tolist()}
    assert len(fwd) == len(u) > 0.5 * len(idx)
    rev = {(b, a, q, p, t) for a, b, p, q, t in fwd}
    assert all(a == b and p == q for a, b, p, q, t in fwd & rev)  # only a self-symmetric key meets its reverse
    # and the flow table agrees: through the oracle's table every kept frame is a miss that reaches the ACL
    hdr, lens, vlan = ac.frames(k, c.macs[u])
    o, _ = oracle_of(c)
    ft = pyoracle.OracleFlow(o, capacity=len(u))
    try:
        r = ft.classify_batch(hdr, lens, cfg=o.cfg(0, 1, NOW))
    finally:
        ft.close()
    hit, act = c.linear(sel=u)
    assert np.array_equal(r["acl_hit"], hit)
    assert np.array_equal(r["verdict"], ac.expected(hit, act, k["proto"] == 6, vlan, flow=True))
