"""A directed collision corpus for the stateful flow table, its plain model and a layout simulator.

Random traffic over a table of at least 2 * (capacity + max_batch) slots almost never fills a 4-slot probe group, lets a
run spill or wrap, leaves a tombstone in front of a live key, has two creators of one 5-tuple in opposite orientations,
or overflows one owner's 16-entry update bucket.  Here every packet is placed to do one of these.

Key search     keys(geom, home, n, proto): n 5-tuples client:sport -> server:80 whose flow_hashfn & gmask is `home`.
               flow_hashfn is tluhash(sip, sport) ^ tluhash(dip, dport) ^ tluhash(proto, 0) (pyoracle's
               oracle_flow_hashfn, pinned to the reference by test_oracle_ref.py), so the two halves are hashed once per
               geometry and joined: a few thousand hash calls even for a 2^22-group mask.  Cached per geometry; nothing
               generated is committed.
FlowModel      one packet at a time in batch order over a dict keyed by the canonical 5-tuple: FlowFind, syn_check, ACL,
               FlowAdd against a free count, direction, FlowUpdate, last-seen; age(now, timeout).  Decode, the tuple and
               the provisional ACL verdict of each packet come from the stateless oracle's row (pinned by their own
               corpora).  No hash table, no probing, no tombstones: it cannot share a layout mistake with the kernels.
LayoutSim      linear probing over groups of 4 with the geometry's mask, tombstones kept until a rehash.  Coverage
               assertions only (does the corpus reach the layout it aims at?), and the tombstone count.  With linear
               probing the set of occupied slots does not depend on the insertion order, so it also holds for flows
               created concurrently in one batch.
families       run, displace, tomb, rehash, age, tuple, order, pool, update (+ the test hooks' forms), each a list of
               cases; a case is a list of steps (a batch with its `now`, or an aging call)."""
from collections import Counter

import numpy as np

import pyoracle
from pktbuild import tcp_packet, udp_packet
from ppe import abi
from ppe.abi import ST

C = {k: i for i, k in enumerate(abi.COUNTERS)}
FW, DROP = abi.ACL_RULE_ACTION_FW, abi.ACL_RULE_ACTION_DROP
FLOWBITS = abi.F_FLOW | abi.F_TOCLIENT | abi.F_NEWFLOW
NOW = 1_000_000
STRIDE = 64
WG = 256            # packets per workgroup of the classify launch in flow mode (4 tiles of 64)
UPD_CAP = 16        # PPE_UPD_CAP: entries per (owner, classify workgroup) bucket
UPD_OWNERS = 256    # PPE_UPD_OWNERS
SYN, SYNACK, ACK = 0x02, 0x12, 0x10


# ---- geometries ----
class Geom:
    """ppe_flow_create's geometry for (capacity, max_batch)."""

    def __init__(self, name, capacity, max_batch):
        self.name, self.capacity, self.max_batch = name, capacity, max_batch
        ns = 64
        while ns < 2 * (capacity + max_batch):
            ns <<= 1
        self.nslots, self.groups, self.gmask = ns, ns // 4, ns // 4 - 1
        osh = 0
        while (ns >> osh) > min(UPD_OWNERS, ns):
            osh += 1
        self.osh, self.owners = osh, ns >> osh

    def __repr__(self):
        return self.name


G64, G1K, G64K = Geom("g64", 16, 16), Geom("g1k", 256, 256), Geom("g64k", 1 << 14, 1 << 14)
GEOMS = {g.name: g for g in (G64, G1K, G64K)}
BIG = Geom("big", 1 << 22, 1 << 15)   # test_gpu_flow.py::test_flow_large_table_global_buckets' table: 2^24 slots
assert (G64.nslots, G1K.nslots, G64K.nslots, BIG.nslots) == (64, 1024, 1 << 16, 1 << 24)
assert (G64.osh, G1K.osh, G64K.osh, BIG.osh) == (0, 2, 8, 16)

# ---- the rule set (first match wins; the default is DROP) ----
X, Y = 0x0AFE0001, 0x0AFE0002            # X -> Y is dropped, Y -> X is not
TNET = 0x0A0A0000                        # 10.10/16: the tuple family's addresses, forwarded on any port
TA, TB, TC = TNET + 1, TNET + 2, TNET + 3
CLIENT, SERVER = 0x0A000001, 0x0B000000  # the searched keys: CLIENT:sport -> SERVER + j : 80


def rules():
    r = np.zeros(7, abi.RULE_DTYPE)
    r["sport_end"] = r["dport_end"] = 65535
    r["protocol_end"] = 255
    r["action"] = FW
    r[0]["sip"], r[0]["sip_mask"], r[0]["dip"], r[0]["dip_mask"], r[0]["action"] = X, 32, Y, 32, DROP
    r[1]["dport_start"] = r[1]["dport_end"] = 80
    r[2]["dip"], r[2]["dip_mask"] = TNET, 16
    r[3]["sip_mask"] = 32                                  # from 0.0.0.0
    r[4]["dip_mask"] = 32                                  # to 0.0.0.0
    r[5]["sip"], r[5]["sip_mask"] = 0xFFFFFFFF, 32
    r[6]["dip"], r[6]["dip_mask"] = 0xFFFFFFFF, 32
    return r


def filler(i):
    """A packet no rule matches (default DROP): it creates no flow and only shifts the directed ones."""
    return udp_packet(0x0C000100 + i, 0x0C000002, 1000 + (i & 0x3FFF), 9)


# ---- key search ----
_halves, _keys = {}, {}


def flow_hash(key):
    sip, dip, sport, dport, proto = key
    return int(pyoracle.load().oracle_flow_hashfn(proto, sip, dip, sport, dport))


def _half(geom):
    """tluhash halves: client side over sports 1024.., server side over SERVER + j, enough pairs for ~48 per group."""
    if geom.name not in _halves:
        na = min(16384, max(64, geom.groups))
        nb = max(16, min(8192, 48 * geom.groups // na))
        h = pyoracle.load().oracle_tluhash
        ha = np.array([h(CLIENT, 1024 + i) for i in range(na)], np.uint32)
        hb = np.array([h(SERVER + j, 80) for j in range(nb)], np.uint32)
        _halves[geom.name] = (ha, hb)
    return _halves[geom.name]


def keys(geom, home, n=24, proto=17):
    """n keys (sip, dip, sport, dport, proto) homed in group `home` of geom, the same ones on every call."""
    k = (geom.name, home, proto)
    if k not in _keys or len(_keys[k]) < n:
        ha, hb = _half(geom)
        hp = np.uint32(pyoracle.load().oracle_tluhash(proto, 0))
        out = []
        for j in range(len(hb)):
            for i in np.flatnonzero(((ha ^ hb[j] ^ hp) & np.uint32(geom.gmask)) == home):
                out.append((CLIENT, SERVER + j, 1024 + int(i), 80, proto))
            if len(out) >= max(n, 24):
                break
        assert len(out) >= n, (geom, home, n, len(out))
        for key in out[:3]:
            assert flow_hash(key) & geom.gmask == home
        _keys[k] = out
    return _keys[k][:n]


def plain_keys(geom, n, avoid):
    """n forwarded keys of no particular home, none homed in a group of `avoid` (the pool family's pool fillers)."""
    out, i = [], 0
    while len(out) < n:
        key = (0x0D000000 + i, SERVER, 2000 + (i & 0x7FFF), 80, 17)
        i += 1
        if flow_hash(key) & geom.gmask not in avoid:
            out.append(key)
    return out


# ---- packets and steps ----
def fwd(key, flags=SYN, payload=22):
    """The key's packet in its own orientation: TCP (54 bytes) or UDP (42 bytes + payload: 64 by default)."""
    sip, dip, sport, dport, proto = key
    return tcp_packet(sip, dip, sport, dport, flags=flags) if proto == 6 else \
        udp_packet(sip, dip, sport, dport, payload=b"\0" * payload)


def rev(key, flags=SYNACK, payload=22):
    sip, dip, sport, dport, proto = key
    return fwd((dip, sip, dport, sport, proto), flags, payload)


def batch(frames, now, wire=None, tag=""):
    """One classify step.  wire: {index: wire length} for frames whose length word differs from the bytes present."""
    hdr = np.zeros((len(frames), STRIDE), np.uint8)
    lens = np.zeros(len(frames), np.uint32)
    for i, f in enumerate(frames):
        assert len(f) <= STRIDE
        hdr[i, :len(f)] = np.frombuffer(f, np.uint8)
        lens[i] = len(f)
    for i, w in (wire or {}).items():
        lens[i] = w
    return dict(kind="batch", hdr=hdr, lens=lens, now=now, tag=tag)


def age(now, timeout=20):
    return dict(kind="age", now=now, timeout=timeout)


def batches(frames, now, geom, tag="", pad=0):
    """frames in batches of at most max_batch, each behind `pad` fillers (so the directed packets lie in a later
    workgroup of the two-launch path)."""
    room = geom.max_batch - pad
    assert room > 0
    return [batch([filler(i) for i in range(pad)] + frames[lo:lo + room], now, tag=tag)
            for lo in range(0, len(frames), room)]


def rolled(frames, geom, pad=0):
    """The same packets in other lanes and tiles: fillers in front (as many as the batch has room for, at most 70), the
    directed ones in reverse order."""
    out = []
    room = geom.max_batch - pad
    step = max(1, room - min(70, room // 4))
    for lo in range(0, len(frames), step):
        part = frames[lo:lo + step][::-1]
        out.append([filler(100 + i) for i in range(room - step)] + part)
    return out


def find_steps(ks, now, geom, pad=0, tag="find"):
    """Every key in both directions, then the rolled form of the same packets."""
    frames = [fwd(k, ACK) for k in ks] + [rev(k, ACK) for k in ks]
    steps = batches(frames, now, geom, tag, pad)
    for fr in rolled(frames, geom, pad):
        steps += batches(fr, now + 1, geom, tag + " rolled", pad)
    return steps


def case(name, geom, steps, capacity=None, env=None, **meta):
    return dict(name=name, geom=geom, steps=steps, capacity=capacity or geom.capacity, env=env or {}, meta=meta)


# ---- the plain model ----
def flow_key(sip, dip, sport, dport, proto):
    """FlowMatch (flow.c:81-94): the 5-tuple in either direction."""
    a, b = (sip, sport), (dip, dport)
    return (proto,) + (a + b if a <= b else b + a)


class FlowModel:
    """flow.c one packet at a time: FlowFind (:96-118, :196-201), syn_check (:204-214), DP_Acl_Lookup (:232-243), FlowAdd
    (:120-158) against the pool's free count, FlowGetPacketDirection (:248-269), FlowUpdate (:163-178), and
    FlowAgeTimeoutCB (:391-467)."""

    def __init__(self, oracle, capacity):
        self.o, self.capacity = oracle, capacity
        self.flows = {}
        self.new_flow = self.del_flow = 0
        self.age_cases = Counter()   # (case, died) of every flow at every aging call

    def classify_batch(self, hdr, lens, now, syn_check=1):
        """verdict, flow_hash, acl_hit, counters (abi.COUNTERS order) and, for the layout simulator and the coverage
        assertions, events: (what, key, index, oriented-as-the-canonical-key)."""
        dec = self.o.classify_batch(hdr, lens, cfg=self.o.cfg(0, syn_check, now))
        verdict, hit = dec["verdict"].copy(), dec["acl_hit"].copy()
        cnt = dec["counters"].astype(np.int64).copy()
        events, born = [], set()   # born: the flows this batch created

        def move(i, st, flags, hitv, deltas):
            verdict[i] = st | ((abi.ACT_FW if st == ST["ACL_FW"] else abi.ACT_DROP) << 8) | (flags << 16)
            hit[i] = hitv
            for k, d in deltas:
                cnt[C[k]] += d

        for i in range(len(lens)):
            v = int(dec["verdict"][i])
            st0, fl = v & 0xFF, v >> 16
            if not fl & abi.F_L4:          # never reached FlowHandlePacket
                continue
            sip, dip, w2, w3 = (int(x) for x in dec["tuple"][i])
            sport, dport, proto = w2 & 0xFFFF, w2 >> 16, w3 & 0xFF
            key = flow_key(sip, dip, sport, dport, proto)
            canon = (sip, sport) <= (dip, dport)
            undo = {ST["ACL_FW"]: [("acl_fw", -1), ("flow_proc_ok", -1), ("out_fw", -1)],
                    ST["ACL_DROP"]: [("acl_drop", -1), ("flow_proc_fail", -1), ("out_drop", -1)],
                    ST["FLOW_TCP_NO_SYN_FIRST"]: [("flow_tcp_no_syn_first", -1), ("flow_proc_fail", -1),
                                                  ("out_drop", -1)]}[st0]
            f = self.flows.get(key)
            if f is not None:              # found: no syn_check, no ACL lookup
                bits = self._update(f, sip, sport, dport, int(lens[i]), now)
                move(i, ST["ACL_FW"], (fl & ~(abi.F_ACL | FLOWBITS)) | bits, -1,
                     undo + [("acl_fw", 1), ("flow_proc_ok", 1), ("out_fw", 1)])
                events.append(("found_new" if key in born else "found", key, i, canon))
                continue
            if st0 != ST["ACL_FW"]:        # TCP without SYN, or the ACL's DROP: the stateless row stands
                continue
            if len(self.flows) >= self.capacity:     # FlowAdd :124-129 (STAT_ACL_FW stays counted, :240)
                move(i, ST["FLOW_NOMEM"], fl, int(dec["acl_hit"][i]),
                     [("flow_proc_ok", -1), ("out_fw", -1), ("flow_node_nomem", 1), ("flow_proc_fail", 1),
                      ("out_drop", 1)])
                events.append(("nomem", key, i, canon))
                continue
            f = dict(sip=sip, dip=dip, sport=sport, dport=dport, protocol=proto, pktcnts2d=0, pktcntd2s=0,
                     bytecnts2d=0, bytecntd2s=0, last_seen=now)
            self.flows[key] = f
            born.add(key)
            self.new_flow += 1
            bits = self._update(f, sip, sport, dport, int(lens[i]), now)
            move(i, ST["ACL_FW"], fl | bits | abi.F_NEWFLOW, int(dec["acl_hit"][i]), [])
            events.append(("new", key, i, canon))
        return dict(verdict=verdict, flow_hash=dec["flow_hash"], acl_hit=hit, tuple=dec["tuple"],
                    counters=cnt.astype(np.uint64), events=events, stateless=dec["verdict"])

    @staticmethod
    def _update(f, sip, sport, dport, wire_len, now):
        to_server = (f["sport"] == sport) if sport != dport else (f["sip"] == sip)
        if sport == f["sport"]:
            f["pktcnts2d"] += 1
            f["bytecnts2d"] += wire_len
        else:
            f["pktcntd2s"] += 1
            f["bytecntd2s"] += wire_len
        f["last_seen"] = now
        return abi.F_FLOW | (0 if to_server else abi.F_TOCLIENT)

    def age(self, now, timeout=20):
        """now > last_seen && now - last_seen > timeout; returns the number deleted (self.dead: their keys)."""
        self.dead = []
        for k, f in self.flows.items():
            d = now - f["last_seen"]
            died = d > 0 and d > timeout
            kind = ("now<L" if d < 0 else "now==L,T0" if d == 0 and timeout == 0 else "now==L" if d == 0 else
                    "T0" if timeout == 0 else "T" if d == timeout else "T+1" if d == timeout + 1 else "other")
            self.age_cases[(kind, died)] += 1
            if died:
                self.dead.append(k)
        for k in self.dead:
            del self.flows[k]
        self.del_flow += len(self.dead)
        return len(self.dead)

    def table(self):
        """The flows as test_gpu_flow.table() lists a dump."""
        cols = ("sip", "dip", "sport", "dport", "protocol", "pktcnts2d", "pktcntd2s", "bytecnts2d", "bytecntd2s",
                "last_seen")
        return sorted(tuple(f[c] for c in cols) for f in self.flows.values())

    def stats(self):
        return dict(live=len(self.flows), new_flow=self.new_flow, del_flow=self.del_flow)


def dump_table(d):
    """A flow dump (ppe_flow_dump / oracle_flow_dump) as FlowModel.table() lists the flows."""
    cols = ("sip", "dip", "sport", "dport", "protocol", "pktcnts2d", "pktcntd2s", "bytecnts2d", "bytecntd2s",
            "last_seen")
    return sorted(tuple(int(x) for x in r) for r in zip(*(d[c] for c in cols)))


# ---- the layout simulator (coverage only) ----
TOMB = "tomb"


class LayoutSim:
    def __init__(self, geom):
        self.g = geom
        self.slot = [None] * geom.nslots   # None = EMPTY, TOMB, or the canonical key
        self.tombs = self.rehashes = 0
        self.seen = Counter()              # the coverage conditions met

    def home(self, key):
        proto, a, ap, b, bp = key
        return flow_hash((a, b, ap, bp, proto)) & self.g.gmask

    def _probe(self, key):
        s0 = 4 * self.home(key)
        for d in range(self.g.nslots):
            yield (s0 + d) % self.g.nslots

    def find(self, key):
        tomb = False
        for s in self._probe(key):
            if self.slot[s] is None:
                return None
            if self.slot[s] == key:
                if tomb:
                    self.seen["live_behind_tomb"] += 1
                return s
            tomb |= self.slot[s] == TOMB
        return None

    def insert(self, key):
        h, tomb = self.home(key), False
        for s in self._probe(key):
            if self.slot[s] is None:
                self.slot[s] = key
                if tomb:
                    self.seen["claim_passes_tomb"] += 1
                g = s // 4
                if all(x is not None for x in self.slot[4 * g:4 * g + 4]):
                    self.seen["full_group"] += 1
                if (g - h) % self.g.groups >= 2:
                    self.seen["run_over_3_groups"] += 1
                if g < h:
                    self.seen["run_wraps"] += 1
                if (s >> self.g.osh) != ((4 * h) >> self.g.osh):
                    self.seen["owner_change_in_run"] += 1
                return s
            tomb |= self.slot[s] == TOMB
        raise AssertionError("table full")

    def kill(self, key):
        self.slot[self.find(key)] = TOMB
        self.tombs += 1

    def revoke(self, key):
        """A refused creator's claim: its slot is taken during the classify launch and left a tombstone."""
        self.slot[self.insert(key)] = TOMB
        self.tombs += 1

    def maybe_rehash(self):
        """flow_maybe_rehash: before every batch and after every aging call."""
        if self.tombs > self.g.nslots // 4:
            live = [k for k in self.slot if k is not None and k != TOMB]
            self.slot = [None] * self.g.nslots
            self.tombs = 0
            for k in live:
                self.insert(k)
            self.rehashes += 1
            self.seen["rehash_due"] += 1

    def apply(self, events):
        """One batch's events: the creators' and the refused creators' claims (each tuple claims once), and per (owner,
        workgroup) the bucket positions of the packets found in the table as it stood before the batch."""
        bucket, refused = Counter(), set()
        for what, key, i, _ in events:
            if what == "found":
                b = (self.find(key) >> self.g.osh, i // WG)
                bucket[b] += 1
                if bucket[b] > UPD_CAP:
                    self.seen["bucket_overflow"] += 1
        for what, key, i, _ in events:
            if what == "new":
                self.insert(key)
            elif what == "nomem" and key not in refused:
                refused.add(key)
        for key in refused:
            self.revoke(key)


def run_model(c, oracle=None):
    """A case through FlowModel and LayoutSim: per step the model's result (a batch's dict, or an aging call's count),
    the table, the stats and the simulator's tombstone count."""
    o = oracle or pyoracle.Oracle(rules(), default_action=DROP)
    m, sim, out = FlowModel(o, c["capacity"]), LayoutSim(c["geom"]), []
    for s in c["steps"]:
        if s["kind"] == "batch":
            assert len(s["lens"]) <= c["geom"].max_batch
            sim.maybe_rehash()
            r = m.classify_batch(s["hdr"], s["lens"], s["now"])
            sim.apply(r["events"])
        else:
            r = m.age(s["now"], s["timeout"])
            for k in m.dead:
                sim.kill(k)
            sim.maybe_rehash()
        out.append(dict(res=r, table=m.table(), stats=m.stats(), tombs=sim.tombs, rehashes=sim.rehashes))
    return out, m, sim


# ---- families ----
def homes(geom):
    return (0, geom.groups // 2 + 1, geom.gmask)


def fam_run(geom, pad=0, kmax=9, ks=None):
    """k keys of one home group, created in one batch (their claims contend for the same EMPTY slots), then found in both
    directions and rolled; and created one key per batch, every key found after each."""
    out = []
    for h in homes(geom):
        K = (ks or keys)(geom, h, kmax)
        for k in range(1, kmax + 1):
            steps = batches([fwd(x) for x in K[:k]], NOW, geom, "create", pad) + find_steps(K[:k], NOW + 1, geom, pad)
            out.append(case(f"run-batch-h{h}-k{k}", geom, steps, home=h, k=k))
        steps = []
        for k in range(1, kmax + 1):
            steps += batches([fwd(K[k - 1])], NOW + 3 * k, geom, "create one", pad)
            frames = [fwd(x) for x in K[:k]] + [rev(x) for x in K[:k]]
            steps += batches(frames, NOW + 3 * k + 1, geom, "find", pad)
        steps += find_steps(K, NOW + 40, geom, pad)
        out.append(case(f"run-serial-h{h}", geom, steps, home=h, k=kmax))
    return out


def fam_displace(geom, pad=0):
    """A run from g spills into g + 1; keys homed in g + 1 then land in g + 2; and the other creation order."""
    out = []
    for g in (geom.groups // 2 + 1, geom.gmask):
        A, B = keys(geom, g, 6), keys(geom, (g + 1) & geom.gmask, 4)
        for name, first, second in (("ab", A, B), ("ba", B, A)):
            steps = batches([fwd(x) for x in first], NOW, geom, "create first", pad) + \
                batches([fwd(x) for x in second], NOW + 1, geom, "create second", pad) + \
                find_steps(A + B, NOW + 2, geom, pad)
            out.append(case(f"displace-{name}-g{g}", geom, steps))
    return out


def fam_tomb(geom, pad=0):
    """A run of 6; keys 1 and 3 aged out (the keepers touched later, the timeout between); the keys behind the tombstones
    found; a new key of the same home created past them; an aged key sent again is a new flow."""
    out = []
    for g in homes(geom):
        K = keys(geom, g, 7)
        keep = [K[0], K[2], K[4], K[5]]
        steps = batches([fwd(x) for x in K[:6]], NOW, geom, "create", pad) + \
            batches([rev(x) for x in keep], NOW + 10, geom, "touch keepers", pad) + [age(NOW + 25, 20)] + \
            find_steps(keep, NOW + 26, geom, pad, "find behind tombstones") + \
            batches([fwd(K[6]), rev(K[1]), fwd(K[1])], NOW + 28, geom, "new key; aged key again", pad) + \
            find_steps(keep + [K[6], K[1]], NOW + 29, geom, pad) + \
            batches([fwd(K[3]), fwd(K[3]), rev(K[3])], NOW + 31, geom, "the other aged key", pad)
        out.append(case(f"tomb-g{g}", geom, steps))
    return out


def fam_rehash(geom=G64, pad=0):
    """g64: a colliding run and a wrapping run kept alive while 5 short-lived keys per cycle are created and aged out,
    until the tombstones pass nslots / 4 and the table is rebuilt; then every keeper is found, counters intact."""
    P = keys(geom, 3, 6) + keys(geom, geom.gmask, 5)
    steps = batches([fwd(x) for x in P], NOW, geom, "create keepers", pad)
    for c in range(5):
        t = NOW + 100 * (c + 1)
        E = keys(geom, 7 + c // 2, 24)[5 * (c % 2):5 * (c % 2) + 5]
        steps += batches([fwd(x) for x in E], t, geom, f"cycle {c} create", pad)
        steps += batches([rev(x) for x in P], t + 10, geom, f"cycle {c} touch keepers", pad)
        steps += [age(t + 25, 20)]
    steps += find_steps(P, NOW + 700, geom, pad)
    return [case("rehash", geom, steps)]


def fam_age(geom, pad=0):
    """A flow last seen at L against now and timeout T: now - L = T (kept) and T + 1 (deleted), now == L, now < L, and
    T == 0 (deleted at now - L = 1, kept at now == L).  A found packet in either direction, and a TCP packet without SYN
    that finds the flow, refresh L."""
    T, L = 20, NOW
    U = keys(geom, 2, 4)
    Tc = keys(geom, 5, 2, proto=6)
    steps = batches([fwd(x) for x in U + Tc], L, geom, "create", pad)
    steps += [age(L + T, T), age(L, T), age(L - 5, T), age(L - 5, 0), age(L, 0)]
    steps += batches([rev(U[1]), fwd(U[2]), fwd(Tc[0], ACK), rev(Tc[1], ACK)], L + 1, geom, "refresh", pad)
    steps += [age(L + T + 1, T)]                       # U[0], U[3]: T + 1, deleted; the refreshed four: T, kept
    steps += find_steps([U[1], U[2], Tc[0], Tc[1]], L + T + 1, geom, pad)
    steps += batches([fwd(U[0])], L + T + 2, geom, "a deleted one again", pad)
    steps += [age(L + T + 3, 0)]                       # rolled finds at L + T + 2: now - L = 1 > 0, all deleted
    return [case("age", geom, steps)]


def swap_ports_pair(geom):
    """Ports p, q such that TA:p -> TB:q and TA:q -> TB:p, two flows that differ only in which port goes with which
    address, are homed in one group: a probe for one compares the other's key."""
    h = pyoracle.load().oracle_tluhash
    x = [h(TA, p) ^ h(TB, p) for p in range(1, 4097)]     # home(p, q) ^ home(q, p) = (x[p] ^ x[q]) & gmask
    seen = {}
    for i, v in enumerate(x):
        if v & geom.gmask in seen:
            p, q = seen[v & geom.gmask] + 1, i + 1
            a, b = (TA, TB, p, q, 17), (TA, TB, q, p, 17)
            assert flow_hash(a) & geom.gmask == flow_hash(b) & geom.gmask and flow_key(*a) != flow_key(*b)
            return a, b
        seen[v & geom.gmask] = i
    raise AssertionError("no colliding port pair")


def proto_twins(geom):
    """A UDP key and the TCP key of the same addresses and ports.  The hash takes the protocol in, so their homes differ
    by a constant XOR d; with the TCP home x = d's top bit, the UDP home is x ^ d, `dist` groups earlier.  4 keys for each
    group between: once they are aged out, their tombstones push the UDP key into the TCP key's home group."""
    h = pyoracle.load().oracle_tluhash
    d = (h(17, 0) ^ h(6, 0)) & geom.gmask
    x = 1 << (d.bit_length() - 1)
    hu = x ^ d
    assert 0 <= hu < x and 4 * (x - hu) <= min(geom.nslots // 4, geom.capacity), (geom, d)
    u = keys(geom, hu, 5)[4]
    t = u[:4] + (6,)
    assert flow_hash(t) & geom.gmask == x
    return u, t, [k for g in range(hu, x) for k in keys(geom, g, 4)]


def fam_tuple(geom, pad=0):
    """Keys that differ only in the protocol (the state word's byte) or in which port goes with which address, placed so
    that a probe for one meets the other; equal addresses and ports; equal ports (direction by address); ports 0 and
    65535, addresses 0 and 0xFFFFFFFF, and the all-zero key."""
    Z = 0xFFFFFFFF
    creators = [
        (TA, TB, 1000, 80, 17), (TA, TB, 1000, 80, 6),                     # UDP and TCP: two flows
        (TA, TB, 1, 2, 17), (TA, TB, 2, 1, 17), (TB, TA, 1, 2, 17),         # two flows: the third is the second's reverse
        (TA, TB, 11, 12, 17),                                              # with its reverse below: one flow
        (TC, TC, 7, 7, 17),                                                # sip == dip, sport == dport
        (TA, TB, 7777, 7777, 17),                                          # sport == dport: direction by address
        (TA, TB, 0, 65535, 17), (0, 0, 0, 0, 17), (0, Z, 65535, 0, 17), (Z, 0, 0, 0, 6),
    ]
    first = [fwd(x) for x in creators] + [rev(creators[5], SYN), rev(creators[7], SYN), fwd(creators[7])]
    steps = batches(first, NOW, geom, "create", pad) + find_steps(creators, NOW + 1, geom, pad)
    out = [case("tuple", geom, steps, flows=len(creators) - 1)]
    # the port-swapped pair in one home group: one in the table when the other arrives, and both new in one batch
    a, b = swap_ports_pair(geom)
    steps = batches([fwd(a)], NOW, geom, "create one of the pair", pad) + \
        batches([fwd(b), rev(b), rev(a), fwd(a), fwd(b)], NOW + 1, geom, "the other arrives", pad) + \
        find_steps([a, b], NOW + 2, geom, pad)
    out.append(case("tuple-swapped-ports", geom, steps))
    steps = batches([fwd(b), fwd(a), rev(a), rev(b)], NOW, geom, "both new in one batch", pad) + \
        find_steps([a, b], NOW + 2, geom, pad)
    out.append(case("tuple-swapped-ports-one-batch", geom, steps))
    # the protocol twins: the UDP flow lies in the TCP key's home group when the SYN arrives
    u, t, fill = proto_twins(geom)
    steps = batches([fwd(x) for x in fill], NOW, geom, "fill the groups between", pad) + [age(NOW + 30, 20)] + \
        batches([fwd(u)], NOW + 31, geom, "the UDP twin, pushed by the tombstones", pad) + \
        batches([fwd(t, ACK), fwd(t, SYN), rev(t, SYNACK), fwd(u), rev(u), fwd(t, ACK)], NOW + 32, geom, "the TCP twin", pad) + \
        find_steps([u, t], NOW + 33, geom, pad)
    out.append(case("tuple-protocol-twins", geom, steps, twins=(u, t)))
    return out


def fam_order(geom, pad=0):
    """One 5-tuple inside one batch: the order of the packets decides who creates and how the flow is oriented."""
    c, s = CLIENT, SERVER + 1
    out = []
    # the reverse direction has no rule (DROP), the forward creator, then both directions; X -> Y is dropped by rule 0
    # and Y -> X creates, so X's packets are the to-client ones
    fr = [udp_packet(s, c, 80, 40002), udp_packet(c, s, 40002, 80), udp_packet(s, c, 80, 40002),
          udp_packet(c, s, 40002, 80), udp_packet(X, Y, 80, 81), udp_packet(Y, X, 81, 80), udp_packet(X, Y, 80, 81),
          udp_packet(Y, X, 81, 80)]
    out.append(case("order-drop-then-create", geom, batches(fr, NOW, geom, "order", pad)))
    # a non-SYN packet ahead of its SYN
    k = (c, s, 40000, 80, 6)
    fr = [fwd(k, ACK), fwd(k, SYN), rev(k, SYNACK), fwd(k, ACK)]
    out.append(case("order-ack-before-syn", geom, batches(fr, NOW, geom, "order", pad)))
    # a creator, then packets of its flow that are no creators themselves (the reverse direction has no rule; TCP
    # without SYN) in other waves, tiles and workgroups: finalize finds their flow by a probe that may meet the slot
    # still PEND or already LIVE
    n = geom.max_batch - pad
    m = min(n, 900)
    ku, kt = (c, s, 40010, 80, 17), (c, s, 40011, 80, 6)
    fr = [filler(i) for i in range(m)]
    fr[min(2, m - 1)], fr[min(3, m - 1)] = fwd(ku), fwd(kt, SYN)
    for j, i in enumerate(range(5, m, max(1, m // 40))):
        fr[i] = (rev(ku), fwd(kt, ACK), rev(kt, ACK), fwd(ku))[j % 4]
    out.append(case("order-found-in-other-tiles", geom, batches(fr, NOW, geom, "order", pad) +
                    find_steps([ku, kt], NOW + 1, geom, pad)))
    # the same with finalize held to one workgroup (PPE_FLOW_FIN_WGS=1: 16 waves) over 64 miss tiles: the creators are in
    # a wave's first tile, their flows' other packets in tiles the waves reach three rounds later, when the slots are
    # LIVE and no longer PEND
    if n >= 4096:
        fr = [filler(i) for i in range(4096)]
        fr[2], fr[3] = fwd(ku), fwd(kt, SYN)
        for j, i in enumerate(range(3080, 4096, 37)):
            fr[i] = (rev(ku), fwd(kt, ACK), rev(kt, ACK), fwd(ku))[j % 4]
        out.append(case("order-found-once-live", geom, batches(fr, NOW, geom, "order", pad) +
                        find_steps([ku, kt], NOW + 1, geom, pad), env={"PPE_FLOW_FIN_WGS": "1"}))
    # would-be creators of one tuple, the lowest index in reverse orientation; later packets in both directions
    a, b = (TA, TB, 1000, 2000, 17), (TB, TA, 2000, 1000, 17)
    forms = {16: [(5, 9, 14)], 256: [(5, 100, 200), (63, 64, 70)]}.get(n, [(5, 300, 700), (250, 256 + 3, 256 + 40)])
    for idx in forms:
        m = min(n, idx[2] + 200)
        fr = [filler(i) for i in range(m)]
        fr[idx[0]], fr[idx[1]], fr[idx[2]] = fwd(b), fwd(a), fwd(a)
        for j, i in enumerate(range(idx[2] + 1, m, max(1, (m - idx[2]) // 6))):
            fr[i] = fwd(a) if j % 2 else fwd(b)
        steps = batches(fr, NOW, geom, "creators", pad) + find_steps([a], NOW + 1, geom, pad)
        out.append(case(f"order-creators-{idx[0]}-{idx[1]}-{idx[2]}", geom, steps, creators=idx))
    return out


def fam_pool(geom, pad=0):
    """k slots of the pool free: exactly k creators of one probe group (all granted), and k + 1 (the last in packet order
    refused, every repeat of it FLOW_NOMEM, a repeat of a granted one found); aging frees the pool and the refused tuple
    creates; the revoked claim's tombstone lies on the run and the keys behind it are still found."""
    out, k = [], 3
    for h in (geom.groups // 2 + 1, geom.gmask):
        K = keys(geom, h, k + 2)
        fill = plain_keys(geom, geom.capacity - k, {(h + d) & geom.gmask for d in range(3)})
        for extra in (0, 1):
            order = [K[2], K[0], K[3], K[1]][:k + extra] if extra else K[:k]
            last = order[-1]
            fr = [fwd(x) for x in order] + [fwd(last), rev(order[0]), rev(last), fwd(order[1]), fwd(last)]
            steps = batches([fwd(x) for x in fill], NOW, geom, "fill the pool", pad) + \
                batches(fr, NOW + 10, geom, "creators", pad) + [age(NOW + 25, 20)] + \
                batches([fwd(K[1]), rev(K[1]), fwd(K[4])], NOW + 26, geom, "the refused tuple creates", pad) + \
                find_steps(K, NOW + 27, geom, pad)
            out.append(case(f"pool-h{h}-k+{extra}", geom, steps, free=k, creators=k + extra))
    return out


def _mixed(i):
    return 65535 if i % 3 == 0 else 60


def fam_update(geom, pad=0, env=None, ks=None):
    """The owner-computed update's 16-entry buckets: one flow found by 15, 16, 17 and 200 packets of one workgroup in
    both directions, wire lengths 60 and 65,535; more than 16 flows of one owner found from one workgroup (g1k: an owner
    is one group, so its 4 flows 5 times each; larger tables: 17 flows once each), and spread over two workgroups."""
    ks = ks or keys
    out = []
    n = min(geom.max_batch - pad, 2 * WG)
    one = ks(geom, 9, 1)[0]
    steps = batches([fwd(one)], NOW, geom, "create", pad)
    for m in (15, 16, 17, 200):
        fr = [filler(i) for i in range(min(n, WG))]
        pos = [(7 * j + 3) % WG for j in range(m)] if m < 100 else list(range(20, 220))
        for j, p in enumerate(pos):   # 60-byte frames; every third one's length word says 65,535
            fr[p] = rev(one, payload=18) if j % 2 else fwd(one, payload=18)
        s = batches(fr, NOW + m, geom, f"one flow x{m}", pad)
        for j, p in enumerate(pos):
            s[0]["lens"][pad + p] = _mixed(j)
        steps += s
    out.append(case("update-one-flow", geom, steps, env=env))
    # Decode reads the low 16 bits of the length word ((uint16_t)pkt_totallen, decode.c:22) and FlowUpdate adds all of
    # it: a word of 65,600 is a 64-byte frame that counts 65,600 bytes.  Such words cannot ride in a 4-byte bucket entry
    # (16 bits), nor, from 2^31, in an 8-byte one: the direct form takes them.
    long_ = ks(geom, 13, 1)[0]
    words = (65600, 0x20040, 0x7FFFFFFF, 0x80000040, 0xFFFFFFFF, 64)
    fr = [filler(i) for i in range(min(n, WG))]
    pos = [(13 * j + 2) % WG for j in range(24)]
    for j, p in enumerate(pos):
        fr[p] = rev(long_) if j % 2 else fwd(long_)
    s = batches([fwd(long_)], NOW, geom, "create with a long length word", pad) + \
        batches(fr, NOW + 1, geom, "length words above 65,535", pad)
    s[0]["lens"][pad] = 65600 + 0x30000
    for j, p in enumerate(pos):
        s[1]["lens"][pad + p] = words[(j // 2) % len(words)]
    out.append(case("update-long-length-words", geom, s, env=env))
    if geom.osh >= 4:     # 17 flows of one owner: homes 64 o .. 64 o + 16 (or the big table's first owner)
        base = 3 << (geom.osh - 2)
        F = [ks(geom, base + j, 1)[0] for j in range(17)]
        reps = 1
    else:                 # one group per owner
        F, reps = ks(geom, 11, 4), 5
    found = [fwd(x) if j % 2 else rev(x) for _ in range(reps) for j, x in enumerate(F)]
    steps = batches([fwd(x) for x in F], NOW, geom, "create", pad)
    fr = [filler(i) for i in range(min(n, WG))]
    for j, f in enumerate(found):
        fr[(11 * j + 5) % WG] = f
    steps += batches(fr, NOW + 1, geom, "one owner, one workgroup", pad)
    if n >= 2 * WG:
        fr = [filler(i) for i in range(2 * WG)]
        for j, f in enumerate(found):
            fr[(j % 2) * WG + 9 * j % WG] = f        # 9 + 8: no bucket overflows
        steps += batches(fr, NOW + 2, geom, "one owner, two workgroups", pad)
        fr = [filler(i) for i in range(2 * WG)]
        for j, f in enumerate(found):
            fr[(5 * j + 1) % WG] = f
            fr[WG + (3 * j + 2) % WG] = f            # 17 in each
        steps += batches(fr, NOW + 3, geom, "one owner, 17 from each of two workgroups", pad)
    out.append(case("update-one-owner", geom, steps, env=env))
    return out


FOLD = {"PPE_FLOW_FOLD_PKTS": "3", "PPE_FLOW_FOLD_BYTES": "500"}


def fam_fold(geom, pad=0):
    """PPE_FLOW_FOLD_PKTS=3 / PPE_FLOW_FOLD_BYTES=500: a flow's d2s direction reaches exactly 2, 3 and 4 packets of 60
    bytes, and exactly 499, 500 and 501 bytes in 2 packets, within one batch and across two."""
    P, B = keys(geom, 4, 6), keys(geom, 6, 6)
    steps = batches([fwd(x) for x in P + B], NOW, geom, "create", pad)
    fr, wire = [], {}
    for j, total in enumerate((2, 3, 4)):
        fr += [rev(P[j])] * total                                 # in one batch
    for j, total in enumerate((499, 500, 501)):
        wire[pad + len(fr)], wire[pad + len(fr) + 1] = 250, total - 250
        fr += [rev(B[j])] * 2
    for j, total in enumerate((2, 3, 4)):
        fr += [rev(P[3 + j])] * (total // 2)                      # across two: the first part
    for j in range(3):
        wire[pad + len(fr)] = 250
        fr += [rev(B[3 + j])]
    s1 = batches(fr, NOW + 1, geom, "fold in one batch; first parts", pad)
    fr2, wire2 = [], {}
    for j, total in enumerate((2, 3, 4)):
        fr2 += [rev(P[3 + j])] * (total - total // 2)
    for j, total in enumerate((499, 500, 501)):
        wire2[pad + len(fr2)] = total - 250
        fr2 += [rev(B[3 + j])]
    s2 = batches(fr2, NOW + 2, geom, "second parts", pad)
    assert len(s1) == 1 and len(s2) == 1
    for s, w in ((s1[0], wire), (s2[0], wire2)):
        for i, v in w.items():
            s["lens"][i] = v
    steps += s1 + s2 + find_steps(P + B, NOW + 3, geom, pad)
    return [case("fold-edges", geom, steps, env=FOLD)]


def fam_update_hooks(geom, pad=0):
    out = []
    for h in ("1", "2"):
        for c in fam_update(geom, pad, env={"PPE_FLOW_UPD_HASH": h}):
            c["name"] += f"-hash{h}"
            out.append(c)
    for c in fam_update(geom, pad, env=FOLD):
        c["name"] += "-fold"
        out.append(c)
    return out + fam_fold(geom, pad)


FAMILIES = {   # name -> (builder, the geometries it makes sense at)
    "run": (fam_run, ("g64", "g1k", "g64k")),
    "displace": (fam_displace, ("g64", "g1k", "g64k")),
    "tomb": (fam_tomb, ("g64", "g1k", "g64k")),
    "rehash": (fam_rehash, ("g64",)),
    "age": (fam_age, ("g64", "g1k", "g64k")),
    "tuple": (fam_tuple, ("g64", "g1k", "g64k")),
    "order": (fam_order, ("g64", "g1k", "g64k")),
    "pool": (fam_pool, ("g64", "g1k")),                 # (filling g64k's pool takes 2^14 flows: not a small test)
    "update": (fam_update, ("g1k", "g64k")),
    "update_hooks": (fam_update_hooks, ("g1k", "g64k")),
}
PAIRS = [(f, g) for f, (_, gs) in FAMILIES.items() for g in gs]
_cases = {}


def cases(family, gname, pad=0):
    k = (family, gname, pad)
    if k not in _cases:
        _cases[k] = FAMILIES[family][0](GEOMS[gname], pad=pad)
    return _cases[k]
