"""Writes tests/golden/flow_stream_portscan_v1.npz: one generated scenario of tests/flow_stream_portscan_model.py (the
attack monitors, FlowGetFlowFromHash with PortScan_Detect inside, then StreamTcp: launch kind 8; ticks and aging between
the batches) frozen as model output only, so that a change of the composition, of the generator or of the models under it
shows (tests/test_flow_stream_portscan_model.py replays it on the CPU, tests/test_gpu_flow_stream_portscan.py on the GPU).

Run from the repository root after the build: python tests/golden/gen_flow_stream_portscan_golden.py"""
import sys
from collections import Counter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle")]

from ppe import abi  # noqa: E402
from test_flow_stream_portscan_model import gen_sequence, run_generated  # noqa: E402

SEED, BATCHES, MAX_N = 137, 12, 96

if __name__ == "__main__":
    seq, par = gen_sequence(SEED, BATCHES, MAX_N)
    ev = Counter()
    outs, m = run_generated(seq, par, 8, ev)
    sess = m.sessions()
    np.savez_compressed(Path(__file__).resolve().parent / "flow_stream_portscan_v1.npz", seed=SEED, batches=BATCHES,
                        max_n=MAX_N,
                        verdict=np.concatenate([o["verdict"] for o, _ in outs]),
                        acl_hit=np.concatenate([o["acl_hit"] for o, _ in outs]),
                        results=np.concatenate([o["results"] for o, _ in outs]),
                        reasons=np.concatenate([r for _, r in outs]),
                        counters=sum(o["counters"] for o, _ in outs),
                        stream_counters=np.array(m.cnt.c, np.uint64),
                        flows=np.array(m.table(), np.uint64).reshape(-1, 10),
                        records=np.array(sorted(m.fp.ps.records()), np.uint64).reshape(-1, 7),
                        sessions=np.array([sum(k, ()) + sess[k] for k in sorted(sess)], np.uint64).reshape(-1, 21),
                        attack=np.array([[a[f] for f in abi.ATTACK_STATE_FIELDS] for a in m.atk.ai], np.uint64))
    print("packets", sum(len(s["lens"]) for s in seq), "events", dict(ev), "flows", len(m.fp.flows), "sessions", len(sess))
