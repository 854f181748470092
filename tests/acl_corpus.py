"""The ACL rule-edge corpus: designed rule sets, keys aimed at every edge of every rule and of every node of the built
classifier image, explicit 64-B frames that carry them, and the expected first match from a plain numpy scan of the
rule table (`linear`: no oracle, no image, no ctypes).

tests/test_acl_corpus.py checks the corpus's promises on the CPU (the oracle's four walkers equal `linear`, every
internal node of every image is entered on both sides of its threshold, the cut lists' positions and slots are all
matched); tests/test_gpu_acl_edges.py runs it through every kernel family.

A key is one row of KEY_DTYPE; `label` says what the key aims at ("r12.dport.hi+1/lo/tcp": rule 12's dport one past its
end, the other fields at their low corner, as TCP; "n7.d1.thr+1/hi": node 7, which splits on dimension 1, one past its
threshold, the other dimensions at the high corner of the node's path interval)."""
from __future__ import annotations

import os

import numpy as np

from ppe import abi, synth
from ppe.abi import RULE_DTYPE

NOW = 1_700_000_000
KEY_DTYPE = np.dtype([("sip", "<u4"), ("dip", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("proto", "u1")])
FIELDS = ("sip", "dip", "sport", "dport", "proto")
WIDTH = {"sip": 32, "dip": 32, "sport": 16, "dport": 16, "proto": 8}
DMAC0 = np.array([0x02, 0x11, 0x22, 0x33, 0x44, 0x55], np.uint8)  # the MACs of a frame no MAC rule aims at
SMAC0 = np.array([0x02, 0x66, 0x77, 0x88, 0x99, 0xAA], np.uint8)


# ---- the reference ---------------------------------------------------------------------------------------------------
def boxes(rules):
    """Inclusive [lo, hi] of every rule in every field, as int64 (a prefix of length m fixes the top m bits)."""
    lo, hi = {}, {}
    for f in ("sip", "dip"):
        m = rules[f + "_mask"].astype(np.int64)
        host = np.where(m >= 32, 0, (np.int64(1) << (32 - np.minimum(m, 32))) - 1)
        lo[f] = rules[f].astype(np.int64) & ~host & 0xFFFFFFFF
        hi[f] = lo[f] | host
    for f, n in (("sport", "sport"), ("dport", "dport"), ("proto", "protocol")):
        lo[f] = rules[n + "_start"].astype(np.int64)
        hi[f] = rules[n + "_end"].astype(np.int64)
    return lo, hi


def linear(rules, used, keys, macs=None, ts=None, default_action=1):
    """First match by lowest rule index: (hit int32, -1 for none; action uint32, the default on a miss).  A rule
    matches iff lo <= key <= hi in every field, its dmac / smac equal the key's when they are not all zero, and
    time_start <= ts <= time_end unless both are zero (csrc/ppe_image.h).  macs: (n, 12) bytes dmac | smac (default:
    DMAC0 | SMAC0); ts: (n,) seconds (default 0)."""
    rules = np.asarray(rules, RULE_DTYPE)
    n = len(keys)
    idx = np.arange(len(rules)) if used is None else np.flatnonzero(np.asarray(used) != 0)
    r = rules[idx]
    lo, hi = boxes(r)
    if macs is None:
        macs = np.tile(np.concatenate([DMAC0, SMAC0]), (n, 1))
    ts = np.zeros(n, np.uint64) if ts is None else np.asarray(ts, np.uint64)
    r_d, r_s = r["dmac"].any(axis=1), r["smac"].any(axis=1)
    r_t = (r["time_start"] != 0) | (r["time_end"] != 0)
    hit = np.full(n, -1, np.int32)
    val = {f: keys[f].astype(np.int64) for f in FIELDS}
    # (only to keep the key x rule tables small: keys go by the top byte of their sip, each group against the rules
    # whose sip range holds an address with that byte, still in index order)
    top = val["sip"] >> 24
    for b in np.unique(top):
        rr = np.flatnonzero((lo["sip"] >> 24 <= b) & (b <= hi["sip"] >> 24))
        group = np.flatnonzero(top == b)
        step = max(64, (1 << 24) // max(1, len(rr)))
        for a in range(0, len(group) if len(rr) else 0, step):
            kk = group[a:a + step]
            ks, kd = val["sip"][kk][:, None], val["dip"][kk][:, None]
            ki, ri = np.nonzero((ks >= lo["sip"][rr]) & (ks <= hi["sip"][rr]) &
                                (kd >= lo["dip"][rr]) & (kd <= hi["dip"][rr]))  # row-major: rules ascend per key
            ki, ri = kk[ki], rr[ri]
            ok = np.ones(len(ki), bool)
            for f in FIELDS[2:]:
                ok &= (val[f][ki] >= lo[f][ri]) & (val[f][ki] <= hi[f][ri])
            ok &= ~r_d[ri] | (macs[ki, 0:6] == r["dmac"][ri]).all(axis=1)
            ok &= ~r_s[ri] | (macs[ki, 6:12] == r["smac"][ri]).all(axis=1)
            ok &= ~r_t[ri] | ((ts[ki] >= r["time_start"][ri]) & (ts[ki] <= r["time_end"][ri]))
            ki, ri = ki[ok], ri[ok]
            first = np.flatnonzero(np.diff(ki, prepend=-1) != 0)  # the first (lowest) rule of every key that has one
            hit[ki[first]] = idx[ri[first]]
    action = np.where(hit >= 0, rules["action"][np.maximum(hit, 0)] if len(rules) else 0,
                      default_action).astype(np.uint32)
    return hit, action


def expected(hit, action, tcp, vlan, flow=False):
    """The verdict word of a well-formed UDP / bare-SYN TCP frame from its first match: only action 1 drops."""
    drop = np.asarray(action) == abi.ACL_RULE_ACTION_DROP
    st = np.where(drop, abi.ST["ACL_DROP"], abi.ST["ACL_FW"]).astype(np.uint32)
    act = np.where(drop, abi.ACT_DROP, abi.ACT_FW).astype(np.uint32)
    fl = np.full(len(hit), abi.F_L4 | abi.F_ACL, np.uint32)
    fl |= np.where(tcp, abi.F_TCP | abi.F_SYN, 0).astype(np.uint32) | np.where(vlan, abi.F_VLAN, 0).astype(np.uint32)
    if flow:  # every frame a flow miss: a forwarded one creates its flow
        fl |= np.where(drop, 0, abi.F_FLOW | abi.F_NEWFLOW).astype(np.uint32)
    return st | act << 8 | fl << 16


# ---- frames ----------------------------------------------------------------------------------------------------------
def frames(keys, macs=None, stride=128, tag_every=4):
    """64-B frames (hdr (n, stride) uint8, len (n,) uint32, vlan (n,) bool) that carry `keys` (protocol 6: a bare SYN;
    17: UDP) and `macs`; every tag_every-th frame has one 802.1Q tag."""
    n = len(keys)
    assert np.isin(keys["proto"], (6, 17)).all(), "only TCP / UDP frames reach the ACL"
    hdr = np.zeros((n, stride), np.uint8)
    rows = np.arange(n)
    vlan = (rows % tag_every) == tag_every - 1
    tcp = keys["proto"] == 6
    hdr[:, 0:6], hdr[:, 6:12] = (DMAC0, SMAC0) if macs is None else (macs[:, 0:6], macs[:, 6:12])

    def put(off, val, nbytes, sel=None):
        """val, big-endian in nbytes bytes, at byte `off` of the rows in `sel` (a mask; default: every row)."""
        at = rows if sel is None else rows[sel]
        off = np.broadcast_to(np.asarray(off), (n,))[at]
        val = np.broadcast_to(np.asarray(val, np.uint64), (n,))[at]
        for b in range(nbytes):
            hdr[at, off + b] = (val >> np.uint64(8 * (nbytes - 1 - b))) & np.uint64(0xFF)

    l3 = np.where(vlan, 18, 14)
    put(12, np.where(vlan, 0x8100, 0x0800), 2)
    put(14, 0x002A, 2, vlan)
    put(16, 0x0800, 2, vlan)
    ip_len = 64 - l3
    hdr[rows, l3] = 0x45
    put(l3 + 2, ip_len, 2)
    put(l3 + 4, rows & 0xFFFF, 2)
    hdr[rows, l3 + 8] = 64
    hdr[rows, l3 + 9] = keys["proto"]
    put(l3 + 12, keys["sip"], 4)
    put(l3 + 16, keys["dip"], 4)
    l4 = l3 + 20
    put(l4, keys["sport"], 2)
    put(l4 + 2, keys["dport"], 2)
    put(l4 + 4, ip_len - 20, 2, ~tcp)  # uh_len
    put(l4 + 4, 1, 4, tcp)  # th_seq; th_ack stays 0
    hdr[rows[tcp], l4[tcp] + 12] = 0x50
    hdr[rows[tcp], l4[tcp] + 13] = 0x02
    put(l4 + 14, 1024, 2, tcp)
    return hdr, np.full(n, 64, np.uint32), vlan


def tuples(keys):
    """The keys as the tuple words of ppe_acl_lookup: sip, dip, sport | dport << 16, proto."""
    t = np.zeros((len(keys), 4), np.uint32)
    t[:, 0], t[:, 1] = keys["sip"], keys["dip"]
    t[:, 2] = keys["sport"].astype(np.uint32) | keys["dport"].astype(np.uint32) << 16
    t[:, 3] = keys["proto"]
    return t


def mac_words(macs):
    """(n, 12) MAC bytes as ppe_acl_lookup's words: dmac bytes 0-3 (little-endian), bytes 4-5, smac likewise."""
    m = np.ascontiguousarray(macs, np.uint8).astype(np.uint32)
    w = np.zeros((len(m), 4), np.uint32)
    for o, c in ((0, 0), (6, 2)):
        w[:, c] = m[:, o] | m[:, o + 1] << 8 | m[:, o + 2] << 16 | m[:, o + 3] << 24
        w[:, c + 1] = m[:, o + 4] | m[:, o + 5] << 8
    return w


# ---- key generators ----------------------------------------------------------------------------------------------------
class Keys:
    """Rows under construction: keys, labels and (optionally) MACs and timestamps."""

    def __init__(self):
        self.rows, self.labels, self.macs, self.ts = [], [], [], []

    def add(self, sip, dip, sport, dport, proto, label, mac=None, ts=0):
        self.rows.append((sip & 0xFFFFFFFF, dip & 0xFFFFFFFF, sport & 0xFFFF, dport & 0xFFFF, proto & 0xFF))
        self.labels.append(label)
        self.macs.append(np.concatenate([DMAC0, SMAC0]) if mac is None else np.asarray(mac, np.uint8))
        self.ts.append(ts)

    def done(self):
        return dict(keys=np.array(self.rows, KEY_DTYPE), labels=np.array(self.labels, object),
                    macs=np.array(self.macs, np.uint8).reshape(-1, 12), ts=np.array(self.ts, np.uint64))


def concat(parts):
    parts = [p for p in parts if len(p["keys"])]
    return {k: np.concatenate([p[k] for p in parts]) for k in ("keys", "labels", "macs", "ts")}


def sample_rules(rules, used, at_least=300, seed=1, only=None):
    """All used rules of a small set; a seeded sample of `at_least` of a large one; or the rules of `only`."""
    if only is not None:
        return np.asarray(only)
    idx = np.arange(len(rules)) if used is None else np.flatnonzero(np.asarray(used) != 0)
    if len(idx) > 1024:
        idx = np.sort(np.random.default_rng(seed).choice(idx, at_least, replace=False))
    return idx


def rule_edges(rules, used=None, at_least=300, seed=1, only=None):
    """Per rule and each of sip / dip / sport / dport: lo - 1, lo, hi, hi + 1 (mod the field width), the other fields
    once at their lo and once at their hi, as TCP and as UDP."""
    lo, hi = boxes(np.asarray(rules, RULE_DTYPE))
    out = Keys()
    for r in sample_rules(rules, used, at_least, seed, only):
        for f in FIELDS[:4]:
            mod = 1 << WIDTH[f]
            for name, v in (("lo-1", lo[f][r] - 1), ("lo", lo[f][r]), ("hi", hi[f][r]), ("hi+1", hi[f][r] + 1)):
                for cname, corner in (("lo", lo), ("hi", hi)):
                    k = {g: int(corner[g][r]) for g in FIELDS[:4]}
                    k[f] = int(v) % mod
                    for pname, proto in (("tcp", 6), ("udp", 17)):
                        out.add(k["sip"], k["dip"], k["sport"], k["dport"], proto, f"r{r}.{f}.{name}/{cname}/{pname}")
    return out.done()


def parse_nodes(img):
    """The node forest of an image (csrc/ppe_image.h): nodes (n, 4) int64, the dimension each node splits on (5: a
    leaf), and its roots as (node index, {dim: (lo, hi)} where the jump root narrows the interval)."""
    img = np.asarray(img, np.uint32)
    off, n = int(img[5]), int(img[2])
    nodes = img[off:off + 4 * n].reshape(n, 4).astype(np.int64)
    index = lambda byte_off: (byte_off - 4 * off) // 16  # noqa: E731
    dim = np.full(n, -1, np.int64)
    roots = []
    jw = int(img[14])
    if jw:
        d, shift, bits = jw & 0xFF, (jw >> 8) & 0xFF, (jw >> 16) & 0xFF
        jt = img[32:32 + (1 << bits)].astype(np.int64)
        ri, rk = index(jt & 0xFFFFFF), jt >> 24
        for b in np.flatnonzero(np.diff(ri, prepend=-1) != 0):  # runs of buckets share a subtree
            e = b
            while e + 1 < len(ri) and ri[e + 1] == ri[b]:
                e += 1
            roots.append((int(ri[b]), {d: (int(b) << shift, ((int(e) + 1) << shift) - 1)}))
            dim[ri[b]] = rk[b]
    else:
        roots.append((0, {}))
        dim[0] = int(img[13]) >> 8
    inner = np.flatnonzero(nodes[:, 0] != 0xFFFFFFFF)
    dim[index(nodes[inner, 1])] = (nodes[inner, 3] >> 8) & 0xFF
    dim[index(nodes[inner, 2])] = (nodes[inner, 3] >> 24) & 0xFF
    nodes[:, 1], nodes[:, 2] = index(nodes[:, 1]), index(nodes[:, 2])
    assert (dim >= 0).all() and ((dim == 5) == (nodes[:, 0] == 0xFFFFFFFF)).all()
    return nodes, dim, roots


def classify_proto(lo, hi, corner):
    """A protocol inside [lo, hi] that reaches the ACL through the decoder (6 or 17) when there is one; the low
    corner prefers 6 and the high one 17, so both occur."""
    inside = [p for p in ((6, 17) if corner == "lo" else (17, 6)) if lo <= p <= hi]
    return inside[0] if inside else (lo if corner == "lo" else hi)


def image_edges(img):
    """A depth-first walk of the image's node forest that carries each path's interval: per internal node, its
    threshold and threshold + 1 in its own dimension, the other dimensions at the two corners of the path's interval
    (the protocol at 6 / 17 where the interval holds one).  Also returns the nodes left out because their threshold
    lies outside their path's interval (then one side cannot be entered), and the nodes a frame can enter on both
    sides: the ones that do not split on the protocol and whose path's protocol interval holds 6 or 17."""
    nodes, dim, roots = parse_nodes(img)
    out, exempt, by_frame = Keys(), [], []
    full = {0: (0, 0xFFFFFFFF), 1: (0, 0xFFFFFFFF), 2: (0, 0xFFFF), 3: (0, 0xFFFF), 4: (0, 0xFF)}
    stack = [(r, {**full, **iv}) for r, iv in roots]
    while stack:
        i, iv = stack.pop()
        d = int(dim[i])
        if d == 5:
            continue
        thr, (lo, hi) = int(nodes[i, 0]), iv[d]
        if lo <= thr < hi:
            if d != 4 and (iv[4][0] <= 6 <= iv[4][1] or iv[4][0] <= 17 <= iv[4][1]):
                by_frame.append(i)
            for cname in ("lo", "hi"):
                k = [iv[g][0] if cname == "lo" else iv[g][1] for g in range(5)]
                if d != 4:
                    k[4] = classify_proto(*iv[4], cname)
                for name, v in (("thr", thr), ("thr+1", thr + 1)):
                    k[d] = v
                    out.add(*k, f"n{i}.d{d}.{name}/{cname}")
        else:
            exempt.append(i)
        stack.append((int(nodes[i, 1]), {**iv, d: (lo, min(hi, thr))}))
        stack.append((int(nodes[i, 2]), {**iv, d: (max(lo, thr + 1), hi)}))
    return out.done(), exempt, by_frame


def node_coverage(img, keys):
    """Walk `keys` through the image's node tree: per node, whether a key entered it equal to its threshold, and
    whether one entered it equal to threshold + 1."""
    nodes, dim, roots = parse_nodes(img)
    k = np.stack([keys[f].astype(np.int64) for f in FIELDS] + [np.zeros(len(keys), np.int64)], axis=1)
    cur = np.zeros(len(keys), np.int64)
    jw = int(np.asarray(img)[14])
    if jw:
        bits = (jw >> 16) & 0xFF
        jt = np.asarray(img, np.uint32)[32:32 + (1 << bits)].astype(np.int64)
        cur = ((jt & 0xFFFFFF) - 4 * int(img[5])) // 16
        cur = cur[k[:, jw & 0xFF] >> ((jw >> 8) & 0xFF)]
    at, past = np.zeros(len(nodes), bool), np.zeros(len(nodes), bool)
    rows = np.arange(len(keys))
    for _ in range(int(np.asarray(img)[10]) + 1):
        thr = nodes[cur, 0]
        live = thr != 0xFFFFFFFF
        v = k[rows, dim[cur]]
        at[cur[live & (v == thr)]] = True
        past[cur[live & (v == thr + 1)]] = True
        cur = np.where(live, np.where(v > thr, nodes[cur, 2], nodes[cur, 1]), cur)
    assert (nodes[cur, 0] == 0xFFFFFFFF).all()
    return at, past, nodes[:, 0] != 0xFFFFFFFF


def proto_edges(rules, used=None, at_least=300, seed=2, only=None):
    """Per rule protocol_start - 1, start, end, end + 1 with the other fields at the rule's low corner: for the tuple
    API (only 6 and 17 reach the ACL through the decoder)."""
    lo, hi = boxes(np.asarray(rules, RULE_DTYPE))
    out = Keys()
    for r in sample_rules(rules, used, at_least, seed, only):
        for name, v in (("lo-1", lo["proto"][r] - 1), ("lo", lo["proto"][r]), ("hi", hi["proto"][r]),
                        ("hi+1", hi["proto"][r] + 1)):
            out.add(int(lo["sip"][r]), int(lo["dip"][r]), int(lo["sport"][r]), int(lo["dport"][r]), int(v) % 256,
                    f"r{r}.proto.{name}")
    return out.done()


def inside_proto(rules, r):
    """6 or 17 inside rule r's protocol range (6 when there is neither: then the rule cannot match a frame)."""
    a, b = int(rules["protocol_start"][r]), int(rules["protocol_end"][r])
    return 6 if a <= 6 <= b or not a <= 17 <= b else 17


def resid_edges(rules, used=None, only=None):
    """Per MAC rule: its low corner with the rule's own MACs (DMAC0 / SMAC0 where the rule leaves one free), then six
    variants per MAC with one bit flipped in one byte (byte b: bit b; bytes 4-5 sit in another image word than 0-3).
    Per time rule: its low corner at ts = start - 1, start, end, end + 1."""
    rules = np.asarray(rules, RULE_DTYPE)
    lo, _ = boxes(rules)
    out = Keys()
    for r in sample_rules(rules, used, len(rules), only=only):
        k = (int(lo["sip"][r]), int(lo["dip"][r]), int(lo["sport"][r]), int(lo["dport"][r]), inside_proto(rules, r))
        has_d, has_s = rules["dmac"][r].any(), rules["smac"][r].any()
        timed = rules["time_start"][r] != 0 or rules["time_end"][r] != 0
        if not (has_d or has_s or timed):
            continue
        own = np.concatenate([rules["dmac"][r] if has_d else DMAC0, rules["smac"][r] if has_s else SMAC0])
        t_in = int(rules["time_start"][r]) if timed else 0
        if has_d or has_s:
            out.add(*k, f"r{r}.mac.own", own, t_in)
            for which, o in (("dmac", 0), ("smac", 6)):
                for b in range(6):
                    m = own.copy()
                    m[o + b] ^= 1 << b
                    if m[o:o + 6].any():  # (an all-zero MAC is a decode error, not an ACL key)
                        out.add(*k, f"r{r}.{which}.byte{b}", m, t_in)
        if timed:
            t0, t1 = int(rules["time_start"][r]), int(rules["time_end"][r])
            for name, t in (("start-1", t0 - 1), ("start", t0), ("end", t1), ("end+1", t1 + 1)):
                if t >= 0:
                    out.add(*k, f"r{r}.time.{name}", own, t)
    return out.done()


# ---- designed rule sets ------------------------------------------------------------------------------------------------
def blank(n):
    """n rules that match everything."""
    r = np.zeros(n, RULE_DTYPE)
    r["sport_end"] = r["dport_end"] = 0xFFFF
    r["protocol_end"] = 0xFF
    return r


def ip(a, b=0, c=0, d=0):
    return a << 24 | b << 16 | c << 8 | d


def extremes():
    """Prefixes, port ranges and protocol ranges at the ends of their fields.  Each group nests its boxes from the
    most specific to the widest inside addresses of its own, so every used, non-empty, first-seen box owns keys;
    actions cycle over 0 / 1 / 2 / 0xFFFF; rules 0 and 9 are unused (used, rule 0 would match everything and drop);
    the last rules repeat earlier boxes with the other action and can never be the first match.
    Returns (rules, used, shadowed rule indices, empty rule indices)."""
    rows = []

    def rule(sip=(0, 0), dip=(0, 0), sport=(0, 0xFFFF), dport=(0, 0xFFFF), proto=(0, 0xFF)):
        rows.append((sip, dip, sport, dport, proto))

    rule()  # 0: unused
    prefixes = [(0, 32), (0, 31), (0xFFFFFFFF, 32), (0xFFFFFFFE, 31), (0, 1), (0x80000000, 1)]
    for p in prefixes:  # 1-6: sip extremes against one destination
        rule(sip=p, dip=(ip(10, 0, 0, 1), 32), proto=(6, 17))
    rule(sip=(0, 0), dip=(ip(10, 0, 0, 2), 32), proto=(6, 17))  # 7: sip /0 (destination of its own)
    rule(sip=(0, 0), dip=(ip(10, 0, 0, 2), 32))  # 8: the same box, every protocol: owns the protocols outside 6-17
    rule(dip=(ip(10, 0, 0, 3), 32))  # 9: unused
    for p in prefixes:  # 10-15: dip extremes against one source
        rule(sip=(ip(10, 0, 1, 1), 32), dip=p, proto=(6, 17))
    rule(sip=(ip(10, 0, 1, 2), 32), dip=(0, 0), proto=(6, 17))  # 16: dip /0
    ports = [(0, 0), (65535, 65535), (0, 65534)]
    for q in ports:  # 17-19: sport extremes
        rule(sip=(ip(11, 0, 0, 1), 32), dip=(ip(11, 0, 0, 2), 32), sport=q)
    rule(sip=(ip(11, 0, 0, 1), 32), dip=(ip(11, 0, 0, 3), 32), sport=(1, 65535))  # 20
    rule(sip=(ip(11, 0, 0, 1), 32), dip=(ip(11, 0, 0, 4), 32), sport=(5, 4))  # 21: empty
    for q in ports:  # 22-24: dport extremes
        rule(sip=(ip(12, 0, 0, 1), 32), dip=(ip(12, 0, 0, 2), 32), dport=q)
    rule(sip=(ip(12, 0, 0, 1), 32), dip=(ip(12, 0, 0, 3), 32), dport=(1, 65535))  # 25
    rule(sip=(ip(12, 0, 0, 1), 32), dip=(ip(12, 0, 0, 4), 32), dport=(65535, 0))  # 26: empty
    for pr in [(0, 0), (255, 255), (0, 5), (7, 16), (6, 17), (18, 255)]:  # 27-32: protocol ranges, nested
        rule(sip=(ip(13, 0, 0, 0), 24), dip=(ip(13, 1, 0, 0), 16), proto=pr)
    # 33-36: corners in several fields at once
    rule(sip=(0, 32), dip=(0xFFFFFFFF, 32), sport=(65535, 65535), dport=(0, 0), proto=(6, 6))
    rule(sip=(0xFFFFFFFF, 32), dip=(0, 32), sport=(0, 0), dport=(65535, 65535), proto=(17, 17))
    rule(sip=(0xFFFFFFFE, 31), dip=(0xFFFFFFFE, 31), sport=(0, 65534), dport=(1, 65535), proto=(6, 17))
    rule(sip=(0, 31), dip=(0, 31), sport=(1, 65535), dport=(0, 65534), proto=(6, 17))
    first_copy = len(rows)
    for src in (1, 3, 12, 17, 23, 31, 33):  # the same boxes again, at a lower priority
        rows.append(rows[src])
    r = blank(len(rows))
    for i, (s, d, sp, dp, pr) in enumerate(rows):
        r["sip"][i], r["sip_mask"][i], r["dip"][i], r["dip_mask"][i] = s[0], s[1], d[0], d[1]
        r["sport_start"][i], r["sport_end"][i], r["dport_start"][i], r["dport_end"][i] = sp[0], sp[1], dp[0], dp[1]
        r["protocol_start"][i], r["protocol_end"][i] = pr
    r["action"] = np.array([0, 1, 2, 0xFFFF], np.uint16)[np.arange(len(rows)) % 4]
    r["action"][0] = 1
    shadowed = np.arange(first_copy, len(rows))
    r["action"][shadowed] = np.where(r["action"][[1, 3, 12, 17, 23, 31, 33]] == 1, 0, 1)
    used = np.ones(len(rows), np.uint8)
    used[[0, 9]] = 0
    return r, used, shadowed, np.array([21, 26])


FIFTEEN_CLUSTERS, FIFTEEN_LEN = 8, 15


def fifteen():
    """Eight clusters of 15 rules over one /24 pair each, told apart by an exact dport alone: with an 11-bit cut
    every cluster is one bucket list of the maximum length."""
    r = blank(FIFTEEN_CLUSTERS * FIFTEEN_LEN)
    c, j = np.divmod(np.arange(len(r)), FIFTEEN_LEN)
    r["sip"], r["sip_mask"] = (10 + c) << 24, 24
    r["dip"], r["dip_mask"] = (20 + c) << 24, 24
    r["dport_start"] = r["dport_end"] = 1000 + j
    r["action"] = (c + j) & 1
    return r


def fifteen_keys():
    """Every cluster's dport 999 .. 1015: a match at every list position, and none on either side."""
    out = Keys()
    for c in range(FIFTEEN_CLUSTERS):
        for dport in range(999, 1000 + FIFTEEN_LEN + 1):
            for proto in (6, 17):
                out.add(ip(10 + c, 0, 0, dport & 0xFF), ip(20 + c, 0, 0, c), 4000 + c, dport, proto,
                        f"c{c}.dport{dport}/{'tcp' if proto == 6 else 'udp'}")
    return out.done()


LEAFLIST_N = 600
LEAFLIST_AIMS = (0, 253, 254, 255, 599, None)


def leaflist():
    """600 rules over one box that only their dmac tells apart (tests/test_acl_build.py::test_long_leaf_list_escape):
    one leaf of 600 candidates, its count in the escaped count word."""
    r = blank(LEAFLIST_N)
    r["sip"], r["sip_mask"] = ip(10), 8
    r["action"] = np.arange(LEAFLIST_N) & 1
    r["dmac"] = leaflist_mac(np.arange(LEAFLIST_N))
    return r


def leaflist_mac(i):
    v = np.asarray(i, np.uint64) + np.uint64(1)
    return np.stack([(v >> np.uint64(8 * b)) & np.uint64(0xFF) for b in range(6)], axis=-1).astype(np.uint8)


def leaflist_keys():
    out = Keys()
    for aim in LEAFLIST_AIMS:
        mac = np.concatenate([leaflist_mac(LEAFLIST_N if aim is None else aim), SMAC0])
        for proto in (6, 17):
            for sip in (ip(10), ip(10, 255, 255, 255), ip(11)):  # the box's two ends, and one past it
                out.add(sip, ip(1, 2, 3, 4), 1, 2, proto, f"aim{aim}.sip{sip:#x}/{proto}", mac)
    return out.done()


TIMEWRAP = (2**32 - 1, 2**32 + 1)


def residual():
    """synth's 300 rules with MAC / time fields on three in ten, then four rules over boxes of their own whose time
    window straddles 2^32, so the 64-bit compare has both image words in play."""
    base = synth.make_rules(300, seed=70, resid_frac=0.3)
    extra = blank(4)
    extra["sip"], extra["sip_mask"] = ip(9, 9, 9, 0) + np.arange(4), 32
    extra["time_start"], extra["time_end"] = TIMEWRAP
    extra["time_end"][1] = 2**33
    extra["time_start"][2] = 1
    extra["smac"][3] = (2, 0, 0, 0, 0, 9)
    extra["action"] = (0, 1, 0, 1)
    return np.concatenate([base, extra])


# ---- kernel families ---------------------------------------------------------------------------------------------------
# the tunings of tests/test_gpu_decode_edges.py's TUNINGS, and the (fetch, image placement) the host-only planner gives
# each rule set under them.  r256 and r4096 repeat that file's columns.  An image without cut lists (leaflist: MAC
# fields) runs a cut-list tuning as the hoist fetch, which the table says out loud.
TUNINGS = [dict(), dict(lds_image=0), dict(pipeline=1), dict(pipeline=3), dict(pipeline=3, lds_image=0),
           dict(pipeline=4), dict(pipeline=5, lds_image=0), dict(pipeline=5, block=256), dict(block=1024)]
_HL, _MG, _NL, _ML = ("hoist", "lds"), ("multi", "global"), ("none", "lds"), ("multi", "lds")
FAMILIES = {
    "r256": [_HL, _MG, _NL, _ML, _MG, _HL, ("cut", "global"), ("cut", "lds"), _HL],
    "r4096": [("cut", "lds"), _MG, ("none", "split"), _ML, _MG, ("hoist", "split"), ("cut", "global"),
              ("cut", "split"), ("hoist", "split")],
    "extremes": [_HL, _MG, _NL, _ML, _MG, _HL, ("cut", "global"), ("cut", "global"), _HL],
    "leaflist": [_HL, _MG, _NL, _ML, _MG, _HL, ("hoist", "global"), ("hoist", "split"), _HL],
}
PLAN_FETCH = {0: "none", 1: "hoist", 3: "multi", 5: "cut"}  # struct ppe_plan's pipe and mode, as ppe_launch_info
PLAN_IMAGE = {0: "global", 1: "lds", 2: "split"}            # names them


# ---- corpora ---------------------------------------------------------------------------------------------------------
SETS = ("r256", "r4096", "resid", "extremes", "fifteen", "leaflist", "r65536")


class Corpus:
    """One rule set with its keys.  `frame` marks the keys a frame can carry (protocol 6 / 17); the rest are for the
    tuple API alone.  Built once per name (and per builder environment: the node forest does not depend on the cut
    variables, which test_acl_corpus checks by rebuilding)."""

    def __init__(self, name):
        self.name = name
        self.used, self.shadowed, self.empty = None, np.zeros(0, int), np.zeros(0, int)
        extra = []
        if name in ("r256", "r4096", "r65536"):
            n = int(name[1:])
            self.rules = synth.make_rules(n, seed=n) if n != 65536 else synth.make_rules(n)
        elif name == "resid":
            self.rules = residual()
        elif name == "extremes":
            self.rules, self.used, self.shadowed, self.empty = extremes()
        elif name == "fifteen":
            self.rules = fifteen()
            extra.append(fifteen_keys())
        elif name == "leaflist":
            self.rules = leaflist()
            extra.append(leaflist_keys())
        else:
            raise KeyError(name)
        self.img = abi.build_image(self.rules, self.used, default_action=1)[0]
        only = [a for a in LEAFLIST_AIMS if a is not None] if name == "leaflist" else None  # (600 copies of one box)
        self.exempt, self.by_frame = [], []
        parts = [rule_edges(self.rules, self.used, only=only)] + extra
        if name != "r65536":  # (the sampled rule edges alone: its forest has more nodes than a corpus should have keys)
            edges, self.exempt, self.by_frame = image_edges(self.img)
            parts.append(edges)
        parts += [proto_edges(self.rules, self.used, only=only), resid_edges(self.rules, self.used, only=only)]
        c = concat(parts)
        self.keys, self.labels, self.macs, self.ts = c["keys"], c["labels"], c["macs"], c["ts"]
        self.n = len(self.keys)
        self.frame = np.isin(self.keys["proto"], (6, 17))
        self._lin = {}

    def linear(self, default_action=1, ts=None, sel=None):
        """(hit, action) of every key (or of keys[sel]) by the numpy scan; ts: None = the corpus's own timestamps, or
        one value for every key (the batch-wide `now`)."""
        key = (default_action, None if ts is None else int(ts))
        if key not in self._lin:
            t = self.ts if ts is None else np.full(self.n, int(ts), np.uint64)
            self._lin[key] = linear(self.rules, self.used, self.keys, self.macs, t, default_action)
        h, a = self._lin[key]
        return (h, a) if sel is None else (h[sel], a[sel])

    def frames(self, stride=128):
        """The frames of the keys marked `frame`: hdr, len, vlan, and their indices into the corpus."""
        idx = np.flatnonzero(self.frame)
        hdr, lens, vlan = frames(self.keys[idx], self.macs[idx], stride)
        return hdr, lens, vlan, idx


_corpora = {}


def corpus(name):
    if name not in _corpora:
        saved = {k: os.environ.pop(k, None) for k in ("PPE_CUT_BITS", "PPE_CUT_LINES", "PPE_CUT", "PPE_COMPACT",
                                                      "PPE_JUMP_BITS")}
        try:
            _corpora[name] = Corpus(name)
        finally:
            os.environ.update({k: v for k, v in saved.items() if v is not None})
    return _corpora[name]


def flow_unique(keys):
    """Indices of the first key of every flow: (sip, sport) <-> (dip, dport) name the same flow."""
    a = keys["sip"].astype(np.uint64) << np.uint64(16) | keys["sport"].astype(np.uint64)
    b = keys["dip"].astype(np.uint64) << np.uint64(16) | keys["dport"].astype(np.uint64)
    canon = np.stack([np.minimum(a, b), np.maximum(a, b), keys["proto"].astype(np.uint64)], axis=1)
    _, first = np.unique(canon, axis=0, return_index=True)
    return np.sort(first)
