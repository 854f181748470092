"""Thin Python handle over one ppe_ctx_t (one GPU).  Every call goes through libppe_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


class PPEError(RuntimeError):
    pass


class Engine:
    def __init__(self, device: int = 0, lib=None):
        self.lib = lib or abi.load()
        self.ctx = C.c_void_p()
        rc = self.lib.ppe_ctx_create(int(device), C.byref(self.ctx))
        if rc != 0:
            raise PPEError(f"ppe_ctx_create(device={device}) failed: {rc} (is a GPU visible?)")
        self.device = int(device)

    # ---- lifecycle ----
    def close(self):
        if self.ctx:
            self.lib.ppe_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            err = self.lib.ppe_last_error(self.ctx)
            raise PPEError(f"{what} failed: {rc}: {err.decode() if err else ''}")

    # ---- rules ----
    def commit(self, rules: np.ndarray, used: np.ndarray | None = None,
               default_action: int = abi.ACL_RULE_ACTION_DROP) -> dict:
        rules = np.ascontiguousarray(rules, dtype=abi.RULE_DTYPE)
        if used is not None:
            used = np.ascontiguousarray(used, dtype=np.uint8)
        st = abi.AclStats()
        rc = self.lib.ppe_rules_commit(self.ctx, rules.ctypes.data if len(rules) else None,
                                       used.ctypes.data if used is not None else None, len(rules),
                                       int(default_action), C.byref(st))
        self._check(rc, "ppe_rules_commit")
        return st.as_dict()

    def stage(self, rules: np.ndarray, used: np.ndarray | None = None,
              default_action: int = abi.ACL_RULE_ACTION_DROP) -> tuple[int, dict]:
        """ppe_rules_stage: build and upload the back classifier without publishing it; returns (token, stats)."""
        rules = np.ascontiguousarray(rules, dtype=abi.RULE_DTYPE)
        if used is not None:
            used = np.ascontiguousarray(used, dtype=np.uint8)
        st = abi.AclStats()
        tok = C.c_uint64(0)
        rc = self.lib.ppe_rules_stage(self.ctx, rules.ctypes.data if len(rules) else None,
                                      used.ctypes.data if used is not None else None, len(rules),
                                      int(default_action), C.byref(st), C.byref(tok))
        self._check(rc, "ppe_rules_stage")
        return tok.value, st.as_dict()

    def publish(self, token: int) -> None:
        """ppe_rules_publish: the staged classifier of `token` runs for later launches."""
        self._check(self.lib.ppe_rules_publish(self.ctx, int(token)), "ppe_rules_publish")

    def image(self) -> np.ndarray:
        n = C.c_uint32(0)
        self._check(self.lib.ppe_acl_image(self.ctx, None, C.byref(n)), "ppe_acl_image")
        out = np.zeros(n.value, np.uint32)
        self._check(self.lib.ppe_acl_image(self.ctx, out.ctypes.data, C.byref(n)), "ppe_acl_image")
        return out

    # ---- classify ----
    @staticmethod
    def cfg(unsupport_proto_action=0, syn_check=1, now_seconds=0) -> abi.Cfg:
        return abi.Cfg(int(unsupport_proto_action), int(syn_check), int(now_seconds))

    def classify_ptrs(self, hdr: int, lens: int, n: int, stride: int, out: dict, cfg: abi.Cfg | None = None,
                      ts: int | None = None, stream: int | None = None):
        """Device-pointer form (ppe_classify): enqueue on `stream` (hipStream_t as int) and return."""
        b = abi.Batch(hdr, lens, ts, int(n), int(stride))
        r = abi.Result(out.get("verdict"), out.get("flow_hash"), out.get("acl_hit"), out.get("fw_idx"),
                       out.get("drop_idx"), out.get("tile_cnt"), out.get("tuple"), out.get("part8"), out.get("packed"))
        rc = self.lib.ppe_classify(self.ctx, C.byref(b), C.byref(r), C.byref(cfg or self.cfg()), stream)
        self._check(rc, "ppe_classify")

    def classify_torch(self, hdr, lens, out: dict, cfg: abi.Cfg | None = None, ts=None, stream=None):
        """Tensors on this engine's GPU; `out` maps output names to torch tensors (or None)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        stride = hdr.shape[1]
        ptrs = {k: (v.data_ptr() if v is not None else None) for k, v in out.items()}
        if ptrs.get("part_idx"):  # partition layout: one list passed as both fw_idx and drop_idx
            ptrs["fw_idx"] = ptrs["drop_idx"] = ptrs.pop("part_idx")
        self.classify_ptrs(hdr.data_ptr(), lens.data_ptr(), lens.numel(), stride, ptrs, cfg,
                           ts.data_ptr() if ts is not None else None, s.cuda_stream)

    def classify_host(self, hdr: np.ndarray, lens: np.ndarray, ts: np.ndarray | None = None,
                      cfg: abi.Cfg | None = None, chunk: int = 0, outputs=("verdict", "flow_hash", "acl_hit"),
                      ordered: bool = False) -> dict:
        """Host-buffer form (ppe_classify_host: pipelined H2D → classify → D2H).  hdr: (n, stride) uint8.
        ordered: ppe_classify_host_ordered, which runs an attached port-scan table's detector (classify_host_ordered)."""
        hdr = np.ascontiguousarray(hdr, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n, stride = hdr.shape
        res = {}
        if "verdict" in outputs:
            res["verdict"] = np.zeros(n, np.uint32)
        if "flow_hash" in outputs:
            res["flow_hash"] = np.zeros(n, np.uint32)
        if "acl_hit" in outputs:
            res["acl_hit"] = np.zeros(n, np.int32)
        if "fw_idx" in outputs:
            res["fw_idx"] = np.zeros(n, np.uint32)
        if "drop_idx" in outputs:
            res["drop_idx"] = np.zeros(n, np.uint32)
        if "tile_cnt" in outputs:
            res["tile_cnt"] = np.zeros((n + 63) // 64, np.uint32)
        if "part_idx" in outputs:  # partition layout: one list passed as both fw_idx and drop_idx
            res["part_idx"] = np.zeros(n, np.uint32)
        if "tuple" in outputs:
            res["tuple"] = np.zeros((n, 4), np.uint32)
        if ts is not None:
            ts = np.ascontiguousarray(ts, dtype=np.uint64)
        b = abi.Batch(hdr.ctypes.data, lens.ctypes.data, ts.ctypes.data if ts is not None else None, n, stride)
        g = lambda k: res[k].ctypes.data if k in res else None  # noqa: E731
        fw, dr = (g("part_idx"), g("part_idx")) if "part_idx" in res else (g("fw_idx"), g("drop_idx"))
        r = abi.Result(g("verdict"), g("flow_hash"), g("acl_hit"), fw, dr, g("tile_cnt"), g("tuple"))
        name = "ppe_classify_host_ordered" if ordered else "ppe_classify_host"
        rc = getattr(self.lib, name)(self.ctx, C.byref(b), C.byref(r), C.byref(cfg or self.cfg()), int(chunk))
        self._check(rc, name)
        return res

    def classify_host_ordered(self, hdr: np.ndarray, lens: np.ndarray, ts: np.ndarray | None = None,
                              cfg: abi.Cfg | None = None, chunk: int = 0,
                              outputs=("verdict", "flow_hash", "acl_hit")) -> dict:
        """ppe_classify_host_ordered: classify_host whose chunks go through one stream in order, so an attached
        port-scan table gives one ppe_classify's verdicts, counters and records whatever `chunk` is."""
        return self.classify_host(hdr, lens, ts, cfg, chunk, outputs, ordered=True)

    # ---- flow table (ppe_flow_*, dataplane/src/flow/flow.c) ----
    def flow_create(self, capacity: int = 0, max_batch: int = 0):
        self._check(self.lib.ppe_flow_create(self.ctx, int(capacity), int(max_batch)), "ppe_flow_create")

    def flow_destroy(self):
        self._check(self.lib.ppe_flow_destroy(self.ctx), "ppe_flow_destroy")

    def classify_flow_torch(self, hdr, lens, out: dict, cfg: abi.Cfg | None = None, ts=None, stream=None):
        """ppe_classify_flow on tensors of this engine's GPU (same `out` convention as classify_torch)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        ptrs = {k: (v.data_ptr() if v is not None else None) for k, v in out.items()}
        if ptrs.get("part_idx"):
            ptrs["fw_idx"] = ptrs["drop_idx"] = ptrs.pop("part_idx")
        b = abi.Batch(hdr.data_ptr(), lens.data_ptr(), ts.data_ptr() if ts is not None else None, lens.numel(),
                      hdr.shape[1])
        r = abi.Result(ptrs.get("verdict"), ptrs.get("flow_hash"), ptrs.get("acl_hit"), ptrs.get("fw_idx"),
                       ptrs.get("drop_idx"), ptrs.get("tile_cnt"), ptrs.get("tuple"), ptrs.get("part8"),
                       ptrs.get("packed"))
        self._check(self.lib.ppe_classify_flow(self.ctx, C.byref(b), C.byref(r), C.byref(cfg or self.cfg()),
                                               s.cuda_stream), "ppe_classify_flow")

    def classify_flow_host_ports(self, hdr, lens, ports=None, ts=None, cfg: abi.Cfg | None = None, chunk: int = 0,
                                 outputs=("verdict", "flow_hash", "acl_hit", "tuple"), out: dict | None = None) -> dict:
        """ppe_classify_flow_host_ports: classify_flow_host with one input-port byte per packet for the flow-attached
        attack monitors (None: port 0 for every packet; the sticky attack_ports table is not read).  ports: a numpy
        uint8 array (staged), or with `out` a torch CPU uint8 tensor (pinned: the zero-copy form may apply; pageable:
        the staged path runs)."""
        return self.classify_flow_host(hdr, lens, ts, cfg, chunk, outputs, out, ports=ports, _ports_call=True)

    def classify_flow_host(self, hdr, lens, ts=None, cfg: abi.Cfg | None = None, chunk: int = 0,
                           outputs=("verdict", "flow_hash", "acl_hit", "tuple"), out: dict | None = None,
                           ports=None, _ports_call: bool = False) -> dict:
        """ppe_classify_flow_host: FlowHandlePacket for a host-resident batch, in chunks through one stream in order
        (one core's results whatever `chunk` is).  hdr (n, stride) uint8, lens, ts: numpy arrays (staged copies), or
        pinned torch CPU tensors together with `out` (name -> pinned tensor), which the kernels then read and write
        directly when the batch fits the table's max_batch.  (ports: classify_flow_host_ports only.)"""
        if ports is not None and not _ports_call:
            raise ValueError("ports: use classify_flow_host_ports")
        if out is not None:  # caller-owned buffers (pinned torch tensors)
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            n, stride = hdr.shape
            b = abi.Batch(ptr(hdr), ptr(lens), ptr(ts), int(n), int(stride))
            r = abi.Result(ptr(out.get("verdict")), ptr(out.get("flow_hash")), ptr(out.get("acl_hit")),
                           ptr(out.get("fw_idx")), ptr(out.get("drop_idx")), ptr(out.get("tile_cnt")),
                           ptr(out.get("tuple")), ptr(out.get("part8")), ptr(out.get("packed")))
            res = out
        else:
            hdr = np.ascontiguousarray(hdr, dtype=np.uint8)
            lens = np.ascontiguousarray(lens, dtype=np.uint32)
            n, stride = hdr.shape
            shapes = {"verdict": (n, np.uint32), "flow_hash": (n, np.uint32), "acl_hit": (n, np.int32),
                      "tuple": ((n, 4), np.uint32), "fw_idx": (n, np.uint32), "drop_idx": (n, np.uint32),
                      "tile_cnt": ((n + 63) // 64, np.uint32), "part8": (n, np.uint8), "packed": (n, np.uint64)}
            res = {k: np.zeros(*shapes[k]) for k in outputs}
            if ts is not None:
                ts = np.ascontiguousarray(ts, dtype=np.uint64)
            g = lambda k: res[k].ctypes.data if k in res else None  # noqa: E731
            b = abi.Batch(hdr.ctypes.data, lens.ctypes.data, ts.ctypes.data if ts is not None else None, n, stride)
            r = abi.Result(g("verdict"), g("flow_hash"), g("acl_hit"), g("fw_idx"), g("drop_idx"), g("tile_cnt"),
                           g("tuple"), g("part8"), g("packed"))
        if _ports_call:
            if ports is None:
                pp = None
            elif hasattr(ports, "data_ptr"):
                if ports.numel() != n:
                    raise ValueError("ports: one byte per packet")
                pp = ports.data_ptr()
            else:
                ports = np.ascontiguousarray(ports, dtype=np.uint8)  # (kept alive by this frame until the call returns)
                if ports.size != n:
                    raise ValueError("ports: one byte per packet")
                pp = ports.ctypes.data
            rc = self.lib.ppe_classify_flow_host_ports(self.ctx, C.byref(b), C.byref(r), C.byref(cfg or self.cfg()),
                                                       int(chunk), pp)
            self._check(rc, "ppe_classify_flow_host_ports")
            return res
        rc = self.lib.ppe_classify_flow_host(self.ctx, C.byref(b), C.byref(r), C.byref(cfg or self.cfg()), int(chunk))
        self._check(rc, "ppe_classify_flow_host")
        return res

    def flow_launch_info(self) -> tuple:
        """ppe_flow_launch_info: (kind, launches) of the last flow batch: (1, 1) the one-launch kernel, (2, 1) the
        one-launch kernel with the port-scan detector inside, (3, 1) that kernel with the flow-attached monitors in it as
        well (flow_combine), (4, 1) the one-launch kernel with the flow-attached monitors in it (chunks of
        classify_flow_host_ports only), (5, 1) the one-launch kernel with the TCP session machine behind it
        (flow_stream), (6, 1) that kernel with the flow-attached monitors in it as well (flow_stream_monitors), (7, 1)
        the one-launch kernel with the port-scan detector inside and the session machine behind it
        (flow_stream_portscan), (8, 1) that kernel with the flow-attached monitors in it as well, (0, 2) the two
        launches, (0, 0) before the first."""
        k, n = C.c_uint32(9), C.c_uint32(9)
        self._check(self.lib.ppe_flow_launch_info(self.ctx, C.byref(k), C.byref(n)), "ppe_flow_launch_info")
        return k.value, n.value

    def flow_portscan_max(self) -> int:
        """ppe_flow_portscan_max: the packets one device flow batch takes with a port-scan table flow-attached."""
        return int(self.lib.ppe_flow_portscan_max())

    def flow_portscan_rounds(self) -> int:
        """ppe_flow_portscan_rounds: resolve rounds of the last flow batch with the detector inside (debug count)."""
        r = C.c_uint32(0)
        self._check(self.lib.ppe_flow_portscan_rounds(self.ctx, C.byref(r)), "ppe_flow_portscan_rounds")
        return r.value

    def flow_combine(self, on: int) -> None:
        """ppe_flow_combine: 1, a flow batch with a port-scan table (able 1) and attack monitors both flow-attached runs
        the monitors, the detector and the table in one launch (flow_launch_info (3, 1)); 0 (a new context), it is
        refused as before.  The context's: flow_destroy leaves it."""
        self._check(self.lib.ppe_flow_combine(self.ctx, int(on)), "ppe_flow_combine")

    def flow_age(self, now: int, timeout: int = 20) -> int:
        d = C.c_uint64(0)
        self._check(self.lib.ppe_flow_age(self.ctx, int(now), int(timeout), C.byref(d)), "ppe_flow_age")
        return d.value

    def flow_info(self) -> dict:
        fi = abi.FlowInfo()
        self._check(self.lib.ppe_flow_info(self.ctx, C.byref(fi)), "ppe_flow_info")
        return fi.as_dict()

    def flow_clear_stat(self):
        self._check(self.lib.ppe_flow_clear_stat(self.ctx), "ppe_flow_clear_stat")

    def flow_dump(self) -> np.ndarray:
        n = C.c_uint32(0)
        self._check(self.lib.ppe_flow_dump(self.ctx, None, 0, C.byref(n)), "ppe_flow_dump")
        out = np.zeros(n.value, abi.FLOW_ENTRY_DTYPE)
        if n.value:
            self._check(self.lib.ppe_flow_dump(self.ctx, out.ctypes.data, n.value, C.byref(n)), "ppe_flow_dump")
        return out

    def acl_lookup_host(self, tuple_: np.ndarray, macs: np.ndarray | None = None, ts: np.ndarray | None = None,
                        now_seconds: int = 0):
        tuple_ = np.ascontiguousarray(tuple_, dtype=np.uint32)
        n = tuple_.shape[0]
        if macs is not None:
            macs = np.ascontiguousarray(macs, dtype=np.uint32)
        if ts is not None:
            ts = np.ascontiguousarray(ts, dtype=np.uint64)
        hit = np.zeros(n, np.int32)
        act = np.zeros(n, np.uint32)
        t = abi.Tuples(tuple_.ctypes.data, macs.ctypes.data if macs is not None else None,
                       ts.ctypes.data if ts is not None else None, n)
        self._check(self.lib.ppe_acl_lookup_host(self.ctx, C.byref(t), hit.ctypes.data, act.ctypes.data,
                                                 int(now_seconds)), "ppe_acl_lookup_host")
        return hit, act

    # ---- counters / timing ----
    def counters(self) -> dict:
        c = abi.Counters()
        self._check(self.lib.ppe_counters_read(self.ctx, C.byref(c)), "ppe_counters_read")
        return c.as_dict()

    def clear_counters(self):
        self._check(self.lib.ppe_counters_clear(self.ctx), "ppe_counters_clear")

    # ---- StreamTcp's first-packet verdict (ppe_stream_tcp_*, stream-tcp.c StreamTcpPacketStateNone) ----
    def stream_tcp(self, track=1, midstream=0, async_oneside=0, reasm=None) -> dict:
        """ppe_stream_tcp_set for later launches (a new context has tracking off); reasm (show text only) follows
        track unless given.  Returns the setting read back."""
        cfg = abi.StreamTcpCfg(int(track), int(midstream), int(async_oneside),
                               int(track if reasm is None else reasm))
        self._check(self.lib.ppe_stream_tcp_set(self.ctx, C.byref(cfg)), "ppe_stream_tcp_set")
        got = abi.StreamTcpCfg()
        self._check(self.lib.ppe_stream_tcp_get(self.ctx, C.byref(got)), "ppe_stream_tcp_get")
        return got.as_dict()

    def stream_counters(self) -> dict:
        c = abi.StreamCounters()
        self._check(self.lib.ppe_stream_counters_read(self.ctx, C.byref(c)), "ppe_stream_counters_read")
        return c.as_dict()

    def clear_stream_counters(self):
        self._check(self.lib.ppe_stream_counters_clear(self.ctx), "ppe_stream_counters_clear")

    # ---- StreamTcp's session state machine behind the flow table (ppe_flow_stream_*, stream-tcp.c StreamTcpPacket) ----
    def flow_stream(self, on: int = 1) -> None:
        """ppe_flow_stream_attach: 1, later flow batches run every TCP packet that has a flow through its flow's session
        (with stream_tcp(track=1, reasm=0); flow_launch_info (5, 1)); every session record is zeroed.  0: the plain
        kernels again.  Needs a flow table."""
        self._check(self.lib.ppe_flow_stream_attach(self.ctx, int(on)), "ppe_flow_stream_attach")

    def flow_stream_monitors(self, on: int) -> None:
        """ppe_flow_stream_monitors: 1, a flow batch with sessions attached and attack monitors flow-attached runs the
        monitors, the table and the sessions in one launch (flow_launch_info (6, 1)), and syncount_accum takes its
        decrements (a completed handshake, a flow aged out in its handshake); 0 (a new context): such a batch is
        refused."""
        self._check(self.lib.ppe_flow_stream_monitors(self.ctx, int(on)), "ppe_flow_stream_monitors")

    def flow_stream_portscan(self, on: int) -> None:
        """ppe_flow_stream_portscan: 1, a flow batch with sessions attached and a port-scan table flow-attached (able 1)
        runs the table, the detector on its misses and the sessions in one launch (flow_launch_info (7, 1)); with attack
        monitors flow-attached as well, and flow_combine and flow_stream_monitors both on, the reference's whole default
        pipeline in one launch ((8, 1)); 0 (a new context): such a batch is refused."""
        self._check(self.lib.ppe_flow_stream_portscan(self.ctx, int(on)), "ppe_flow_stream_portscan")

    def flow_stream_max(self) -> int:
        """ppe_flow_stream_max: the packets one device flow batch takes with sessions attached."""
        return int(self.lib.ppe_flow_stream_max())

    def flow_stream_dump(self) -> list:
        """ppe_flow_stream_dump: every live TCP flow's key and session record (abi.FlowStreamEntry), in table order."""
        n = C.c_uint32(0)
        self._check(self.lib.ppe_flow_stream_dump(self.ctx, None, 0, C.byref(n)), "ppe_flow_stream_dump")
        out = (abi.FlowStreamEntry * max(1, n.value))()
        if n.value:
            self._check(self.lib.ppe_flow_stream_dump(self.ctx, out, n.value, C.byref(n)), "ppe_flow_stream_dump")
        return list(out[:n.value])

    def stream_track_counters(self) -> dict:
        """ppe_stream_track_counters_read: the 58 fields of tcpstream_track_stat the session path counts, by name."""
        c = abi.StreamTrackCounters()
        self._check(self.lib.ppe_stream_track_counters_read(self.ctx, C.byref(c)), "ppe_stream_track_counters_read")
        return c.as_dict()

    def clear_stream_track_counters(self):
        self._check(self.lib.ppe_stream_track_counters_clear(self.ctx), "ppe_stream_track_counters_clear")

    # ---- port-scan detector (ppe_portscan_*, dataplane/src/attack/dp_portscan.c) ----
    def portscan(self, attach: bool = True, **cfg) -> "PortScan":
        """ppe_portscan_create (cfg: the words of ppe_portscan_cfg_t; none given = the reference's defaults) and, unless
        attach is false, ppe_portscan_attach: later ppe_classify / ppe_classify_batches launches run the detector.
        attach="flow": ppe_flow_portscan_attach instead: later ppe_classify_flow calls run it on flow misses; the
        stateless calls then run without it."""
        ps = PortScan(self, **cfg)
        if attach == "flow":
            ps.attach_flow()
        elif attach:
            ps.attach()
        return ps

    # ---- attack monitors (ppe_attack_*, dataplane/src/attack/dp_attack.c) ----
    def attack(self, cfg: "abi.AttackCfg | None" = None, attach: "bool | str" = True) -> "Attack":
        """ppe_attack_create (cfg None: all-zero rules, hold 600 s) and, unless attach is false, ppe_attack_attach: later
        ppe_classify / ppe_classify_batches launches run the land, SYN-flood and UDP-flood monitors.  attach="flow":
        ppe_flow_attack_attach instead: later ppe_classify_flow calls run them, syncount_accum counting the flows SYNs
        create; the stateless calls then run without monitors."""
        a = Attack(self, cfg)
        if attach == "flow":
            a.attach_flow()
        elif attach:
            a.attach()
        return a

    def timing(self, on: bool = True):
        self._check(self.lib.ppe_timing_enable(self.ctx, 1 if on else 0), "ppe_timing_enable")

    def timing_read(self, reset: bool = True):
        ms = C.c_double()
        n = C.c_uint32()
        self._check(self.lib.ppe_timing_read(self.ctx, C.byref(ms), C.byref(n), 1 if reset else 0),
                    "ppe_timing_read")
        return ms.value, n.value

    def tuning(self, **kw) -> dict:
        """Read (and with keyword arguments, set) the launch tuning: block, blocks_per_cu, pipeline, lds_image."""
        t = abi.Tuning()
        self._check(self.lib.ppe_get_tuning(self.ctx, C.byref(t)), "ppe_get_tuning")
        if kw:
            for k, v in kw.items():
                setattr(t, k, int(v))
            self._check(self.lib.ppe_set_tuning(self.ctx, C.byref(t)), "ppe_set_tuning")
        return t.as_dict()

    def launch_info(self) -> dict:
        g, b, l, v = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.ppe_launch_info(self.ctx, C.byref(g), C.byref(b), C.byref(l), C.byref(v)),
                    "ppe_launch_info")
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value,
                "image": ("global", "lds", "split")[v.value & 15], "fetch": {0: "none", 1: "hoist", 3: "multi", 5: "cut"}.get(v.value >> 4, f"v{v.value >> 4}")}

    def sync(self):
        self._check(self.lib.ppe_sync(self.ctx), "ppe_sync")


def decode_verdict(v: np.ndarray):
    v = np.asarray(v, dtype=np.uint32)
    return v & 0xFF, (v >> 8) & 0xFF, v >> 16


class Defrag:
    """One device FCB table (ppe_defrag_create) on an Engine's GPU: IPv4 reassembly of the fragments ppe_classify
    PUNTs (dataplane/src/decode/decode-defrag.c).  Every call goes through libppe_hip.so."""

    def __init__(self, engine: Engine, fcb_max=0, cache_max=0, frag_buf_bytes=0, reasm_buf_bytes=0, max_batch=0):
        self.eng = engine
        self.lib = engine.lib
        self.h = C.c_void_p()
        cfg = abi.DefragCfg(fcb_max, cache_max, frag_buf_bytes, reasm_buf_bytes, max_batch, 0)
        rc = self.lib.ppe_defrag_create(engine.ctx, C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise PPEError(f"ppe_defrag_create failed: {rc}")
        self.info_ = self.info()

    def close(self):
        if self.h:
            self.lib.ppe_defrag_destroy(self.h)
            self.h = C.c_void_p()

    def _check(self, rc, what):
        if rc != 0:
            err = self.lib.ppe_defrag_last_error(self.h)
            raise PPEError(f"{what} failed: {rc}: {err.decode() if err else ''}")

    def alloc_out(self, n: int, hdr_stride: int = 128, full: bool = True):
        """Device output tensors for a batch of n fragments."""
        import torch
        dev = torch.device("cuda", self.eng.device)
        cm = self.info_["cache_max"]
        out = dict(status=torch.empty(n, dtype=torch.int32, device=dev),
                   dgram_of=torch.empty(n, dtype=torch.int32, device=dev),
                   dgram_hdr=torch.empty((n, hdr_stride), dtype=torch.uint8, device=dev),
                   dgram_len=torch.empty(n, dtype=torch.int32, device=dev),
                   dgram_frags=torch.empty((n, cm), dtype=torch.int64, device=dev),
                   n_dgram=torch.zeros(1, dtype=torch.int32, device=dev))
        if full:
            out["dgram_pkt"] = torch.empty((n, self.info_["reasm_buf_bytes"]), dtype=torch.uint8, device=dev)
        return out

    def run_torch(self, pkt, off, lens, out: dict, now: int, ids=None, stream=None):
        """ppe_defrag on tensors of the engine's GPU: pkt (u8 arena), off (i64), lens (i32), ids (i64, optional)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(self.eng.device)
        n = lens.numel()
        b = abi.FragBatch(pkt.data_ptr(), off.data_ptr(), lens.data_ptr(), ids.data_ptr() if ids is not None else None,
                          n, 0, int(now))
        g = lambda k: out[k].data_ptr() if out.get(k) is not None else None
        o = abi.DefragOut(g("status"), g("dgram_of"), g("dgram_hdr"), g("dgram_len"), g("dgram_pkt"),
                          g("dgram_frags"), g("n_dgram"), out["dgram_hdr"].shape[1], 0)
        self._check(self.lib.ppe_defrag(self.h, C.byref(b), C.byref(o), s.cuda_stream), "ppe_defrag")

    def launch_info(self):
        """(kind, launches) of the last ppe_defrag batch: (1, 1) the one-launch kernel, (0, 6) the six launches."""
        k, l = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.ppe_defrag_launch_info(self.h, C.byref(k), C.byref(l)), "ppe_defrag_launch_info")
        return k.value, l.value

    def run_host(self, pkt, off, lens, now: int, ids=None, chunk: int = 0, hdr_stride: int = 128, full: bool = True,
                 guard: int = 0):
        """ppe_defrag_host on numpy arrays in host memory: pkt (u8 arena), off (u64), lens (u32), ids (u64, optional).
        Returns a dict of numpy outputs (status, dgram_of, dgram_hdr, dgram_len, dgram_frags, n_dgram, and dgram_pkt
        when full), each with `guard` more entries / rows behind its n, filled with 0xA5 bytes."""
        pkt = np.ascontiguousarray(pkt, np.uint8)
        off = np.ascontiguousarray(off, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint32)
        ids = np.ascontiguousarray(ids, np.uint64) if ids is not None else None
        n, cm = int(lens.size), self.info_["cache_max"]
        rows = n + guard
        mk = lambda shape, dt: np.frombuffer(bytearray(b"\xa5" * (int(np.prod(shape)) * np.dtype(dt).itemsize)),
                                             dtype=dt).reshape(shape)
        out = dict(status=mk((rows,), np.uint32), dgram_of=mk((rows,), np.uint32),
                   dgram_hdr=mk((rows, hdr_stride), np.uint8), dgram_len=mk((rows,), np.uint32),
                   dgram_frags=mk((rows, cm), np.uint64), n_dgram=mk((1 + guard,), np.uint32))
        if full:
            out["dgram_pkt"] = mk((rows, self.info_["reasm_buf_bytes"]), np.uint8)
        b = abi.FragBatch(pkt.ctypes.data, off.ctypes.data, lens.ctypes.data,
                          ids.ctypes.data if ids is not None else None, n, 0, int(now))
        g = lambda k: out[k].ctypes.data if k in out else None
        o = abi.DefragOut(g("status"), g("dgram_of"), g("dgram_hdr"), g("dgram_len"), g("dgram_pkt"),
                          g("dgram_frags"), g("n_dgram"), hdr_stride, 0)
        self._check(self.lib.ppe_defrag_host(self.h, C.byref(b), C.byref(o), int(chunk)), "ppe_defrag_host")
        return out

    def age(self, now: int, timeout: int = 20):
        """Frag_defrag_timeout: returns (dropped fragment ids, FCBs freed)."""
        cap = self.info_["fcb_max"] * self.info_["cache_max"]
        ids = np.zeros(cap, np.uint64)
        nd, nf = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.ppe_defrag_age(self.h, int(now), int(timeout), ids.ctypes.data, cap, C.byref(nd),
                                            C.byref(nf)), "ppe_defrag_age")
        return ids[:min(nd.value, cap)], nf.value

    def info(self) -> dict:
        fi = abi.DefragInfo()
        self._check(self.lib.ppe_defrag_info(self.h, C.byref(fi)), "ppe_defrag_info")
        return fi.as_dict()



class PortScan:
    """One port-scan table (ppe_portscan_create) on an Engine's GPU: PortScan_Detect on the stateless classify path
    (dataplane/src/attack/dp_portscan.c).  Every call goes through libppe_hip.so."""

    def __init__(self, engine: Engine, **cfg):
        self.eng = engine
        self.lib = engine.lib
        self.h = C.c_void_p()
        c = None
        if cfg:
            d = dict(able=1, action=0, exception_freq=50, hold_seconds=600, capacity=0, max_batch=0, cycles_per_second=0)
            unknown = set(cfg) - set(d)
            if unknown:
                raise TypeError(f"unknown ppe_portscan_cfg_t words: {sorted(unknown)}")
            d.update(cfg)
            c = abi.PortScanCfg(**{k: int(v) for k, v in d.items()})
        rc = self.lib.ppe_portscan_create(engine.ctx, C.byref(c) if c is not None else None, C.byref(self.h))
        if rc != 0:
            raise PPEError(f"ppe_portscan_create failed: {rc}")

    def _check(self, rc, what):
        if rc != 0:
            err = self.lib.ppe_portscan_last_error(self.h)
            raise PPEError(f"{what} failed: {rc}: {err.decode() if err else ''}")

    def attach(self):
        self.eng._check(self.lib.ppe_portscan_attach(self.eng.ctx, self.h), "ppe_portscan_attach")
        self.eng.portscan_attached = self

    def detach(self):
        self.eng._check(self.lib.ppe_portscan_attach(self.eng.ctx, None), "ppe_portscan_attach")
        self.eng.portscan_attached = None

    def attach_flow(self):
        """ppe_flow_portscan_attach: ppe_classify_flow / _flow_host run the detector on flow misses (batches of at most
        Engine.flow_portscan_max() packets on the device); the engine's stateless calls do not see the table."""
        self.eng._check(self.lib.ppe_flow_portscan_attach(self.eng.ctx, self.h), "ppe_flow_portscan_attach")
        self.eng.portscan_flow_attached = self

    def detach_flow(self):
        self.eng._check(self.lib.ppe_flow_portscan_attach(self.eng.ctx, None), "ppe_flow_portscan_attach")
        self.eng.portscan_flow_attached = None

    def close(self):
        if self.h:
            self.lib.ppe_portscan_destroy(self.h)  # (detaches it first, from whichever point holds it)
            if getattr(self.eng, "portscan_attached", None) is self:
                self.eng.portscan_attached = None
            if getattr(self.eng, "portscan_flow_attached", None) is self:
                self.eng.portscan_flow_attached = None
            self.h = C.c_void_p()

    def clock(self, now_cycles: int, now_seconds: int):
        """cvmx_get_cycle() and OCT_TIME_SECONDS_SINCE1970 for the batches enqueued from now on."""
        self._check(self.lib.ppe_portscan_clock(self.h, int(now_cycles), int(now_seconds)), "ppe_portscan_clock")

    def set(self, **kw) -> dict:
        """able / action / exception_freq / hold_seconds, live; the words not given keep their values."""
        cur = self.info()["cfg"]
        cur.update({k: int(v) for k, v in kw.items()})
        c = abi.PortScanCfg(**cur)
        self._check(self.lib.ppe_portscan_set(self.h, C.byref(c)), "ppe_portscan_set")
        return self.info()["cfg"]

    def age(self, now_cycles: int) -> int:
        """PortScan_timeout: returns the records freed."""
        freed = C.c_uint64(0)
        self._check(self.lib.ppe_portscan_age(self.h, int(now_cycles), C.byref(freed)), "ppe_portscan_age")
        return freed.value

    def prepass_info(self) -> tuple:
        """(kind, launches) of the last batch's pre-pass: kind 1 the one-launch kernel, 0 the staged launches."""
        kind, launches = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.ppe_portscan_prepass_info(self.h, C.byref(kind), C.byref(launches)),
                    "ppe_portscan_prepass_info")
        return kind.value, launches.value

    def info(self) -> dict:
        i = abi.PortScanInfo()
        self._check(self.lib.ppe_portscan_info(self.h, C.byref(i)), "ppe_portscan_info")
        return i.as_dict()

    def dump(self) -> np.ndarray:
        n = C.c_uint32(0)
        self._check(self.lib.ppe_portscan_dump(self.h, None, 0, C.byref(n)), "ppe_portscan_dump")
        ent = np.zeros(n.value, abi.PORTSCAN_ENTRY_DTYPE)
        if n.value:
            self._check(self.lib.ppe_portscan_dump(self.h, ent.ctypes.data, n.value, C.byref(n)), "ppe_portscan_dump")
        return ent


class Attack:
    """The attack monitors of one Engine (ppe_attack_create): land, SYN flood, SYN count and UDP flood on the stateless
    classify path (attach) or on the flow-table path (attach_flow), one of the two at a time
    (dataplane/src/attack/dp_attack.c).  Every call goes through libppe_hip.so."""

    def __init__(self, engine: Engine, cfg: "abi.AttackCfg | None" = None):
        self.eng = engine
        self.lib = engine.lib
        self.h = C.c_void_p()
        self._ports = None  # keeps the caller's port arrays alive while they are in force
        rc = self.lib.ppe_attack_create(engine.ctx, C.byref(cfg) if cfg is not None else None, C.byref(self.h))
        if rc != 0:
            raise PPEError(f"ppe_attack_create failed: {rc}")

    def _check(self, rc, what):
        if rc != 0:
            err = self.lib.ppe_attack_last_error(self.h)
            raise PPEError(f"{what} failed: {rc}: {err.decode() if err else ''}")

    def attach(self):
        self.eng._check(self.lib.ppe_attack_attach(self.eng.ctx, self.h), "ppe_attack_attach")
        self.eng.attack_attached = self

    def detach(self):
        self.eng._check(self.lib.ppe_attack_attach(self.eng.ctx, None), "ppe_attack_attach")
        self.eng.attack_attached = None

    def attach_flow(self):
        """ppe_flow_attack_attach: ppe_classify_flow runs the monitors; the engine's stateless calls do not see them."""
        self.eng._check(self.lib.ppe_flow_attack_attach(self.eng.ctx, self.h), "ppe_flow_attack_attach")
        self.eng.attack_flow_attached = self

    def detach_flow(self):
        self.eng._check(self.lib.ppe_flow_attack_attach(self.eng.ctx, None), "ppe_flow_attack_attach")
        self.eng.attack_flow_attached = None

    def close(self):
        if self.h:
            self.lib.ppe_attack_destroy(self.h)  # (detaches it first, from whichever point holds it)
            if getattr(self.eng, "attack_attached", None) is self:
                self.eng.attack_attached = None
            if getattr(self.eng, "attack_flow_attached", None) is self:
                self.eng.attack_flow_attached = None
            self.h = C.c_void_p()

    def set(self, cfg: "abi.AttackCfg"):
        """The rule file load (and flood_hold_time): ordered with the launches enqueued before and after."""
        self._check(self.lib.ppe_attack_set(self.h, C.byref(cfg)), "ppe_attack_set")

    def clock(self, now_seconds: int):
        self._check(self.lib.ppe_attack_clock(self.h, int(now_seconds)), "ppe_attack_clock")

    def tick(self, now_seconds: int):
        """DP_Attack_Info_Update, once a second in the reference."""
        self._check(self.lib.ppe_attack_tick(self.h, int(now_seconds)), "ppe_attack_tick")

    def ports(self, arrays):
        """arrays: per batch a torch uint8 cuda tensor (one input-port byte per packet) or None; None clears."""
        arrays = list(arrays) if arrays is not None else []
        tab = (C.c_void_p * max(1, len(arrays)))(*[(t.data_ptr() if t is not None else None) for t in arrays])
        self._check(self.lib.ppe_attack_ports(self.h, tab if arrays else None, len(arrays)), "ppe_attack_ports")
        self._ports = arrays

    def info(self) -> dict:
        i = abi.AttackInfo()
        self._check(self.lib.ppe_attack_info(self.h, C.byref(i)), "ppe_attack_info")
        return i.as_dict()

    def info_struct(self) -> "abi.AttackInfo":
        i = abi.AttackInfo()
        self._check(self.lib.ppe_attack_info(self.h, C.byref(i)), "ppe_attack_info")
        return i

    def clear_stat(self):
        self._check(self.lib.ppe_attack_clear_stat(self.h), "ppe_attack_clear_stat")
