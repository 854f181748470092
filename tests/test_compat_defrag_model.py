"""tests/compat_defrag_model.py (the serial model of a Decode flush with defrag_able == 1) pinned by hand-derived hook
sequences, and its promise about the corpus: the frames of tests/defrag_corpus.py give every status Defrag behind
Decode can give them and at least one datagram to each of the fw and the drop hook.  No GPU."""
from collections import Counter

import numpy as np

from compat_defrag_model import DecodeDefragModel
from pktbuild import ip_frag, udp, udp_packet
from ppe import abi

import defrag_corpus as dfc

S, D, NOW = 0x0A000001, 0x0A000002, 1000
DF = abi.DF


def web_rules():
    """TCP or UDP to port 80 forwards; everything else takes the default action, DROP."""
    r = np.zeros(1, abi.RULE_DTYPE)
    r["sport_end"] = 65535
    r["protocol_end"] = 255
    r["dport_start"], r["dport_end"] = 80, 80
    r["action"] = abi.ACL_RULE_ACTION_FW
    return r


def halves(dport, ident=7, sip=S):
    """A UDP datagram of 8 + 24 bytes in two fragments: bytes [0, 16) with MF, bytes [16, 32) without."""
    l4 = udp(1000, dport, bytes(range(24)))
    return (ip_frag(17, sip, D, ident, 0, True, l4[:16]), ip_frag(17, sip, D, ident, 16, False, l4[16:])), l4


def test_two_fragments_in_order_and_reversed():
    (f0, f1), l4 = halves(80)
    for first, second, chain in ((f0, f1, [0, 1]), (f1, f0, [1, 0])):
        m = DecodeDefragModel(web_rules())
        try:
            assert m.flush([first], [0], NOW) == []                       # cached: no hook
            assert m.flush([second], [1], NOW) == [("fw", ("dgram", 1))]  # the datagram in its completing fragment's place
            d = m.dgrams[1]
            assert d["chain"] == chain                                    # offset order: the head first
            assert d["frame"][34:] == l4 and len(d["frame"]) == 14 + 20 + 32
            assert d["frame"][16:18] == bytes([0, 52]) and d["frame"][20:22] == bytes(2)   # ip_len 20 + 32, ip_off 0
        finally:
            m.close()


def test_both_fragments_in_one_burst_between_whole_packets():
    (f0, f1), _ = halves(80)
    web, other = udp_packet(dport=80), udp_packet(dport=81)
    m = DecodeDefragModel(web_rules())
    try:
        ev = m.flush([web, f0, other, f1, web], [0, 1, 2, 3, 4], NOW)
        assert ev == [("fw", 0), ("log", 2), ("drop", 2), ("fw", ("dgram", 3)), ("fw", 4)]
        assert m.dgrams[3]["chain"] == [1, 3]
        # defrag_able 0: today's Decode punts the fragments
        assert m.flush([f0, f1], [5, 6], NOW, defrag_able=0) == [("punt", 5), ("punt", 6)]
    finally:
        m.close()


def test_teardrop_is_dropped_without_a_log():
    l4 = udp(1000, 80, bytes(range(24)))
    f0 = ip_frag(17, S, D, 9, 0, True, l4[:16])
    over = ip_frag(17, S, D, 9, 8, True, l4[8:24])          # bytes [8, 24) over the cached [0, 16)
    m = DecodeDefragModel(web_rules())
    try:
        assert m.flush([f0], [0], NOW) == []
        assert m.flush([over], [1], NOW) == [("drop", 1)]
        assert m.status[1] == DF["DEFRAG_ERR"] | abi.DF_TEARDROP
    finally:
        m.close()


def test_cache_full_is_logged():
    """defrag_cache_max 8: the ninth fragment of a datagram that cannot complete (no first fragment) finds the cache
    full: DP_Log_Func and the drop hook (decode-defrag.c:431-438)."""
    l4 = bytes(range(80))
    fr = [ip_frag(17, S, D, 11, 8 * k, True, l4[8 * k:8 * k + 8]) for k in range(1, 10)]
    m = DecodeDefragModel(web_rules())
    try:
        assert m.flush(fr[:8], list(range(8)), NOW) == []
        assert m.flush(fr[8:], [8], NOW) == [("log", 8), ("drop", 8)]
        assert m.status[8] == DF["CACHE_FULL"]
    finally:
        m.close()


def test_a_datagram_the_acl_drops():
    (f0, f1), _ = halves(81)
    m = DecodeDefragModel(web_rules())
    try:
        assert m.flush([f0, f1], [0, 1], NOW) == [("log", ("dgram", 1)), ("drop", ("dgram", 1))]
        assert m.dgrams[1]["verdict"] & 0xFF == abi.ST["ACL_DROP"] and m.dgrams[1]["chain"] == [0, 1]
    finally:
        m.close()


def test_aging_of_a_held_fragment():
    (f0, f1), _ = halves(80)
    m = DecodeDefragModel(web_rules())
    try:
        assert m.flush([f0], [0], NOW) == []
        assert m.age(NOW + 20) == []                        # idle == FRAG_MAX_TIMEOUT: kept
        assert m.age(NOW + 21) == [("drop", 0)]
        assert m.flush([f1], [1], NOW + 21) == []           # a new FCB: cached again
    finally:
        m.close()


def test_the_corpus_reaches_every_status_and_both_hooks():
    """The corpus's 274 frames through one table of the shim's shape (1,024 FCBs, 8 fragments each, default buffers),
    default action FW: every status Defrag can give them behind Decode (FCB_FULL needs more than 1,024 FCBs and a frame
    Decode does not hold for a fragment never reaches Defrag, so NOT_FRAG cannot occur), datagrams to the fw and to the
    drop hook, whatever the burst."""
    frames = [fr[:n] for c in dfc.cases() for fr, n in c.frames]
    assert len(frames) == 274
    seen = []
    for burst in (1, 64, 300):
        m = DecodeDefragModel(np.zeros(0, abi.RULE_DTYPE), default_action=0)
        try:
            ev = []
            for b in range(0, len(frames), burst):
                ev += m.flush(frames[b:b + burst], list(range(b, min(b + burst, len(frames)))), NOW)
            st = Counter(s & 0xFF for s in m.status.values())
            assert set(st) == {DF[k] for k in ("CACHED", "REASM", "SETUP_ERR", "HW2SW_ERR", "DELETED", "CACHE_FULL",
                                               "DEFRAG_ERR")}
            hooks = Counter(h for h, who in ev if isinstance(who, tuple))
            assert hooks["fw"] >= 1 and hooks["drop"] >= 1 and hooks["fw"] + hooks["drop"] == st[DF["REASM"]]
            seen.append((st, hooks, len(m.age(NOW + 100))))
        finally:
            m.close()
    assert seen[0] == seen[1] == seen[2]    # Defrag is sequential and the datagrams' classify stateless


def test_fcb_full_past_1024_keys():
    """1,030 first fragments of different datagrams: DEFRAG_FCB_MAX is 1,024, so the last six find no FCB and go to the
    drop hook without a log (decode-defrag.c:472-477), whatever the burst."""
    l4 = udp(1000, 80, bytes(range(24)))
    heads = [ip_frag(17, S + 16 + k, D, 500, 0, True, l4[:16]) for k in range(1030)]
    for burst in (300, 1030):
        m = DecodeDefragModel(web_rules())
        try:
            ev = []
            for b in range(0, 1030, burst):
                ev += m.flush(heads[b:b + burst], list(range(b, min(b + burst, 1030))), NOW)
            assert ev == [("drop", k) for k in range(1024, 1030)]
            assert all(m.status[k] == DF["FCB_FULL"] for k in range(1024, 1030))
        finally:
            m.close()
