"""A deterministic corpus of frames on both sides of every comparator of the per-packet decode (helper, no tests).

corpus() is the cross product  L2 tagging x IPv4 header length x (protocol, one mutation)  plus the Ethernet / VLAN
edges of a plain frame, every frame built from explicit bytes; expected() is what the engine must return for it at a
given header window: the oracle's answer on the 256-B window, and for a frame whose decode needs a byte past the
window the engine's own WINDOW_PUNT verdict (include/ppe_hip.h)."""
import struct

import numpy as np

from ppe import abi, synth
from ppe.abi import ST
from pktbuild import eth, ipv4, udp, vlan

WIDTH = 256                                   # the widest header window of the ABI
L2S = ("untagged", "tag8100", "tag9100")
IHLS = tuple(range(5, 16))
PAY = b"\xc3\x3c\xa5\x5a"                     # L4 payload of an unmutated frame
TAIL = b"\x5a\xa5\x69\x96\x0f\xf0\x33"        # Ethernet padding bytes (non-zero on purpose)

ANY_MUTS = ("none", "pad1", "pad7", "cut1", "iplen+1", "iplen<hlen", "len+65536", "off2000", "off0001", "off4000",
            "off8000", "ver5")
TCP_MUTS = ("flags10", "flags12", "flags04", "flags01", "flags00_ack", "doff4", "doff0", "doff6_l4len24",
            "doff6_l4len23", "doff15_l4len60", "doff15_l4len59", "doff8_l4len40", "l4len20", "l4len19", "l4len0")
UDP_MUTS = ("uhlen+1", "uhlen-1", "uhlen+256", "l4len8", "l4len7", "l4len0")
OTHER_MUTS = ("none", "mf", "mf_nopayload")   # protocols 1 and 89


def _tcp(sport, dport, flags=0x02, doff=5, ack=0, l4len=24):
    """A TCP segment of exactly l4len bytes: header, doff * 4 - 20 option bytes (NOPs, then a window-scale option where
    four bytes fit), payload; cut where l4len is shorter than that."""
    nopt = max(0, doff * 4 - 20)
    opts = (b"\x01" * (nopt - 3) + b"\x03\x03\x07") if nopt >= 4 else b"\x01" * nopt
    seg = struct.pack(">HHIIBBHHH", sport, dport, 0x01020304, ack, doff << 4, flags, 1024, 0, 0) + opts
    seg += PAY * 16
    return seg[:l4len]


def _l2(kind, inner, dmac, smac):
    if kind == "untagged":
        return eth(inner, dmac, smac)
    return eth(0x8100 if kind == "tag8100" else 0x9100, dmac, smac) + vlan(inner)


def _frame(l2, ihl, proto, mut, f):
    """One frame of the cross product: (bytes, wire length).  f = the row's addresses and ports."""
    off, ver, extra, ip_len = 0, 4, 0, None
    if proto == 6:
        kw = {"flags10": dict(flags=0x10), "flags12": dict(flags=0x12), "flags04": dict(flags=0x04),
              "flags01": dict(flags=0x01), "flags00_ack": dict(flags=0x00, ack=0x00010000), "doff4": dict(doff=4),
              "doff0": dict(doff=0), "doff6_l4len24": dict(doff=6, l4len=24), "doff6_l4len23": dict(doff=6, l4len=23),
              "doff15_l4len60": dict(doff=15, l4len=60), "doff15_l4len59": dict(doff=15, l4len=59),
              "doff8_l4len40": dict(doff=8, l4len=40), "l4len20": dict(l4len=20), "l4len19": dict(l4len=19),
              "l4len0": dict(l4len=0)}.get(mut, {})
        l4 = _tcp(f["sport"], f["dport"], **kw)
    elif proto == 17:
        l4len = {"l4len8": 8, "l4len7": 7, "l4len0": 0}.get(mut, 8 + len(PAY))
        ulen = l4len + {"uhlen+1": 1, "uhlen-1": -1, "uhlen+256": 256}.get(mut, 0)
        l4 = udp(f["sport"], f["dport"], PAY, ulen=ulen)[:l4len]
    else:
        l4 = b"" if mut == "mf_nopayload" else PAY * 2
        off = 0x2000 if mut in ("mf", "mf_nopayload") else 0
    if proto in (6, 17):
        off = {"off2000": 0x2000, "off0001": 0x0001, "off4000": 0x4000, "off8000": 0x8000}.get(mut, 0)
        ver = 5 if mut == "ver5" else 4
        if mut == "iplen+1":
            ip_len = ihl * 4 + len(l4) + 1
        elif mut == "iplen<hlen":
            ip_len = ihl * 4 - 1
    fr = _l2(l2, 0x0800, f["dmac"], f["smac"]) + ipv4(proto, f["sip"], f["dip"], len(l4), ihl=ihl, ver=ver,
                                                       ip_len=ip_len, off=off) + l4
    if proto in (6, 17):
        if mut in ("pad1", "pad7"):
            fr += TAIL[:int(mut[3:])]
        elif mut == "cut1":
            fr = fr[:-1]
        elif mut == "len+65536":
            extra = 65536
    return fr, len(fr) + extra


def _edges(f):
    """Ethernet and VLAN edges of a plain frame: (name, l2, bytes, wire length)."""
    def plain(l2="untagged", inner=0x0800, dmac=f["dmac"], smac=f["smac"], verhl=0x45):
        l4 = udp(f["sport"], f["dport"], PAY)
        ip = bytearray(ipv4(17, f["sip"], f["dip"], len(l4)))
        ip[0] = verhl
        return _l2(l2, inner, dmac, smac) + bytes(ip) + l4
    out = []
    for n in (0, 13, 14, 15, 33, 34):
        out.append((f"len{n}", "untagged", plain(), n))
    for n in (14, 17, 18, 21, 22, 37, 38):
        out.append((f"tag_len{n}", "tag8100", plain("tag8100"), n))
    out.append(("dmac0", "untagged", plain(dmac=bytes(6)), None))
    out.append(("smac0", "untagged", plain(smac=bytes(6)), None))
    out.append(("etype86dd", "untagged", plain(inner=0x86DD), None))
    for inner in (0x8100, 0x9100, 0x0806):
        fr = plain("tag8100", inner)
        if inner != 0x0806:  # a second tag, then the plain frame's IPv4
            fr = fr[:18] + vlan(0x0800) + fr[18:]
        for n in (None, 21, 22):
            out.append((f"inner{inner:04x}" + (f"_len{n}" if n else ""), "tag8100", fr, n))
    out.append(("ihl0", "untagged", plain(verhl=0x40), None))
    out.append(("ihl4", "untagged", plain(verhl=0x44), None))
    return [(name, l2, fr, len(fr) if n is None else n) for name, l2, fr, n in out]


def corpus(rules, seed=1, reverse=False):
    """(hdr[n, 256] u8, len[n] u32, meta).  Frame k takes its MACs, addresses and ports from row k % 4096 of a synth
    batch drawn for `rules` (so ACL outcomes are non-trivial); reverse swaps the addresses and the ports of every
    frame.  meta: per-frame arrays name, l2, ihl, proto, mut."""
    pk = synth.make_packets(4096, rules, seed, kind="udp64", malformed_frac=0, hit_frac=0.8)
    h = pk["hdr"]

    def row(k):
        r = h[k % 4096]
        f = dict(dmac=bytes(r[0:6]), smac=bytes(r[6:12]), sip=int.from_bytes(bytes(r[26:30]), "big"),
                 dip=int.from_bytes(bytes(r[30:34]), "big"), sport=int.from_bytes(bytes(r[34:36]), "big"),
                 dport=int.from_bytes(bytes(r[36:38]), "big"))
        if reverse:
            f.update(sip=f["dip"], dip=f["sip"], sport=f["dport"], dport=f["sport"])
        return f

    frames, meta = [], []
    protos = [(6, m) for m in ANY_MUTS + TCP_MUTS] + [(17, m) for m in ANY_MUTS + UDP_MUTS] + \
             [(p, m) for p in (1, 89) for m in OTHER_MUTS]
    for l2 in L2S:
        for ihl in IHLS:
            for proto, mut in protos:
                frames.append(_frame(l2, ihl, proto, mut, row(len(frames))))
                meta.append((f"{l2}/ihl{ihl}/proto{proto}/{mut}", l2, ihl, proto, mut))
    for name, l2, fr, n in _edges(row(len(frames))):
        frames.append((fr, n))
        meta.append((f"edge/{name}", l2, 5, 17, name))
    hdr = np.zeros((len(frames), WIDTH), np.uint8)
    lens = np.zeros(len(frames), np.uint32)
    for k, (fr, n) in enumerate(frames):
        assert len(fr) <= WIDTH
        hdr[k, :len(fr)] = np.frombuffer(fr, np.uint8)
        lens[k] = n
    cols = list(zip(*meta))
    m = dict(name=np.array(cols[0]), l2=np.array(cols[1]), ihl=np.array(cols[2]), proto=np.array(cols[3]),
             mut=np.array(cols[4]))
    return hdr, lens, m


def expected(oracle, hdr256, lens, stride, cfg, ts=None, wide=None):
    """What the engine returns for these frames through a stride-wide window.  verdict / flow_hash / acl_hit: the
    oracle on the 256-B window; where the decode needs a byte past the window (reach > stride) the engine's verdict:
    WINDOW_PUNT | PUNT << 8 | (F_VLAN for a tagged frame) << 16, flow hash 0, hit -1.  tuple: the oracle on the
    stride-wide window (PPE_TUPLE_OPT_PAST depends on the width); of a punted frame only addresses and protocol are
    defined (tuple_mask).  counters: the oracle's 32 over the frames not punted, and per punted frame (one that reached
    the L4 decoder) pkts, window_punt, out_punt, l2_rx_ok, ipv4_rx_ok, vlan_rx_ok if tagged, its length in rx_bytes.
    wide: the oracle's result on the 256-B window, when the caller has it already."""
    if wide is None:
        wide = oracle.classify_batch(hdr256, lens, ts=ts, cfg=cfg)
    punt = wide["reach"] > stride
    tagged = ((wide["verdict"] >> 16) & abi.F_VLAN) != 0
    exp = {k: wide[k].copy() for k in ("verdict", "flow_hash", "acl_hit")}
    exp["verdict"][punt] = ST["WINDOW_PUNT"] | (2 << 8) | (np.where(tagged[punt], abi.F_VLAN, 0) << 16)
    exp["flow_hash"][punt] = 0
    exp["acl_hit"][punt] = -1
    narrow = wide if stride == hdr256.shape[1] else oracle.classify_batch(
        np.ascontiguousarray(hdr256[:, :stride]), lens, ts=ts, cfg=cfg)
    exp["tuple"] = narrow["tuple"].copy()
    exp["tuple_mask"] = np.full((len(lens), 4), 0xFFFFFFFF, np.uint32)
    exp["tuple_mask"][punt] = (0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFF)
    exp["tuple"] &= exp["tuple_mask"]
    exp["punt"] = punt
    exp["counters"] = expected_counters(oracle, hdr256, lens, punt, tagged, cfg, ts) if punt.any() \
        else wide["counters"].copy()
    return exp


def expected_counters(oracle, hdr256, lens, punt, tagged, cfg, ts=None):
    """The 32 counters of a batch of which the frames `punt` do not fit the window (see expected)."""
    keep = ~punt
    c = oracle.classify_batch(hdr256[keep], lens[keep], ts=None if ts is None else ts[keep], cfg=cfg)["counters"]
    C = {n: i for i, n in enumerate(abi.COUNTERS)}
    for name in ("pkts", "window_punt", "out_punt", "l2_rx_ok", "ipv4_rx_ok"):
        c[C[name]] += int(punt.sum())
    c[C["vlan_rx_ok"]] += int((punt & tagged).sum())
    c[C["rx_bytes"]] += int(lens[punt].astype(np.uint64).sum())
    return c


def assert_matches(got, exp, meta, what="", keys=("verdict", "flow_hash", "acl_hit", "tuple")):
    """got (engine outputs over the corpus, or a slice of it with exp / meta sliced alike) equals exp, naming the
    first frames that differ by their axes."""
    for k in keys:
        g, e = got[k], exp[k]
        if k == "tuple":
            g = g & exp["tuple_mask"]
        if not np.array_equal(g, e):
            bad = np.nonzero((g != e).reshape(len(e), -1).any(axis=1))[0]
            first = [(int(i), str(meta["name"][i]), np.asarray(g[i]).tolist(), np.asarray(e[i]).tolist())
                     for i in bad[:4]]
            raise AssertionError(f"{what} {k}: {len(bad)} frames differ, first (index, frame, engine, expected): "
                                 f"{first}")


def counters_list(cnt):
    """Engine.counters() in the order of the oracle's counter array."""
    return [int(cnt[n]) for n in abi.COUNTERS]
