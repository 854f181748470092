"""The decode edge corpus (tests/decode_corpus.py) keeps its promises, checked on the CPU against the oracle: every
decode status occurs, the IPv4-options slow path reaches the ACL with both outcomes, frames sit on both sides of the
header-window rule at 64 and 80 bytes, and a narrower window changes nothing for a frame that fits it."""
import numpy as np
import pytest

import pyoracle
from ppe import abi, synth

import decode_corpus as dc

NOW = 1_700_000_000


@pytest.fixture(scope="module")
def world():
    rules = synth.make_rules(256, seed=256)
    hdr, lens, meta = dc.corpus(rules)
    o = pyoracle.Oracle(rules, default_action=1)
    wide = {syn: o.classify_batch(hdr, lens, cfg=o.cfg(0, syn, NOW)) for syn in (1, 0)}
    return rules, hdr, lens, meta, o, wide


def test_corpus_is_deterministic_and_named(world):
    rules, hdr, lens, meta, _, _ = world
    h2, l2, m2 = dc.corpus(rules)
    assert np.array_equal(hdr, h2) and np.array_equal(lens, l2) and np.array_equal(meta["name"], m2["name"])
    assert hdr.shape == (len(lens), 256) and hdr.dtype == np.uint8 and lens.dtype == np.uint32
    assert len(set(meta["name"].tolist())) == len(lens)  # every frame names its own edge
    # the cross product is complete: every L2 tagging x header length x (protocol, mutation)
    per = len(dc.ANY_MUTS) * 2 + len(dc.TCP_MUTS) + len(dc.UDP_MUTS) + 2 * len(dc.OTHER_MUTS)
    for l2 in dc.L2S:
        for ihl in dc.IHLS:
            assert ((meta["l2"] == l2) & (meta["ihl"] == ihl) & ~np.char.startswith(meta["name"], "edge/")).sum() == per
    # reverse swaps addresses and ports, nothing else: the frames differ exactly in those bytes
    hr, lr, _ = dc.corpus(rules, reverse=True)
    assert np.array_equal(lr, lens)
    k = int(np.nonzero(meta["name"] == "untagged/ihl5/proto17/none")[0][0])
    assert bytes(hr[k, 26:30]) == bytes(hdr[k, 30:34]) and bytes(hr[k, 30:34]) == bytes(hdr[k, 26:30])
    assert bytes(hr[k, 34:36]) == bytes(hdr[k, 36:38]) and bytes(hr[k, 36:38]) == bytes(hdr[k, 34:36])
    assert np.array_equal(np.delete(hr[k], np.s_[26:38]), np.delete(hdr[k], np.s_[26:38]))


def test_every_status_occurs(world):
    *_, wide = world
    st1 = set((wide[1]["verdict"] & 0xFF).tolist())
    st0 = set((wide[0]["verdict"] & 0xFF).tolist())
    assert st1 == set(range(18)), sorted(set(range(18)) - st1)
    assert st0 == set(range(17)), sorted(set(range(17)) - st0)


def test_slow_path_reaches_the_acl_with_both_outcomes(world):
    _, _, _, meta, _, wide = world
    for syn in (1, 0):
        acl = ((wide[syn]["verdict"] >> 16) & abi.F_ACL) != 0
        slow = acl & (meta["ihl"] > 5)
        hits = slow & (wide[syn]["acl_hit"] >= 0)
        assert hits.sum() >= 100 and (slow & ~hits).sum() >= 100, (syn, hits.sum(), slow.sum())
        for proto in (6, 17):
            assert (hits & (meta["proto"] == proto)).any() and (slow & ~hits & (meta["proto"] == proto)).any()


def test_frames_on_both_sides_of_the_window_rule(world):
    _, _, _, meta, _, wide = world
    reach = wide[1]["reach"]
    for stride in (64, 80):
        for proto in (6, 17):
            p = meta["proto"] == proto
            assert (p & (reach == stride)).any(), (stride, proto)
            assert (p & (reach > stride)).any(), (stride, proto)
    assert reach.max() <= 92  # so strides >= 96 never punt
    assert np.array_equal(reach, wide[0]["reach"])


@pytest.mark.parametrize("stride", [64, 80, 96, 128])
def test_narrow_window_equals_wide_where_it_fits(world, stride):
    _, hdr, lens, meta, o, wide = world
    for syn in (1, 0):
        nar = o.classify_batch(np.ascontiguousarray(hdr[:, :stride]), lens, cfg=o.cfg(0, syn, NOW))
        fits = wide[syn]["reach"] <= stride
        assert fits.all() == (stride >= 96)
        for k in ("verdict", "flow_hash", "acl_hit"):
            bad = np.nonzero(fits & (nar[k] != wide[syn][k]))[0]
            assert len(bad) == 0, (k, meta["name"][bad[:4]].tolist())


def test_expected_punts_and_counters(world):
    """expected(): at a window with punts the counters still account for every frame and byte, a punted frame gets the
    engine's verdict word, and at a window without punts everything is the oracle's own."""
    _, hdr, lens, meta, o, wide = world
    C = {n: i for i, n in enumerate(abi.COUNTERS)}
    for stride, npunt in ((64, True), (80, True), (96, False), (256, False)):
        e = dc.expected(o, hdr, lens, stride, o.cfg(0, 1, NOW), wide=wide[1])
        assert e["punt"].any() == npunt
        c = e["counters"]
        assert c[C["pkts"]] == len(lens) and c[C["rx_bytes"]] == int(lens.astype(np.uint64).sum())
        assert c[C["out_fw"]] + c[C["out_drop"]] + c[C["out_punt"]] == len(lens)
        assert c[C["window_punt"]] == e["punt"].sum()
        p = e["punt"]
        assert ((e["verdict"][p] & 0xFFFF) == (abi.ST["WINDOW_PUNT"] | (2 << 8))).all()
        assert np.array_equal((e["verdict"][p] >> 16) != 0, meta["l2"][p] != "untagged")
        if not npunt:
            assert np.array_equal(c, wide[1]["counters"])
            for k in ("verdict", "flow_hash", "acl_hit"):
                assert np.array_equal(e[k], wide[1][k])
