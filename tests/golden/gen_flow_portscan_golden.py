"""Writes tests/golden/flow_portscan_v1.npz: one generated scenario of tests/flow_portscan_model.py (FlowGetFlowFromHash
with PortScan_Detect inside, small pools, a stepped clock, aging between the batches) frozen as model output only, so
that a change of the model, of the generator or of the oracle under them shows (tests/test_flow_portscan_model.py replays
it).

Run from the repository root after the build: python tests/golden/gen_flow_portscan_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "packet-process-engine_amd"), str(ROOT / "oracle")]

import flow_portscan_model as fpm  # noqa: E402
from test_flow_portscan_model import run_generated  # noqa: E402

SEED, BATCHES, MAX_N = 77, 40, 96

if __name__ == "__main__":
    seq, par = fpm.gen_sequence(SEED, BATCHES, MAX_N)
    outs, m = run_generated(seq, par)
    np.savez_compressed(Path(__file__).resolve().parent / "flow_portscan_v1.npz", seed=SEED, batches=BATCHES, max_n=MAX_N,
                        verdict=np.concatenate([o["verdict"] for o in outs]),
                        acl_hit=np.concatenate([o["acl_hit"] for o in outs]),
                        results=np.concatenate([o["results"] for o in outs]),
                        counters=sum(o["counters"] for o in outs),
                        flows=np.array(m.table(), np.uint64).reshape(-1, 10),
                        records=np.array(sorted(m.ps.records()), np.uint64).reshape(-1, 7))
    print("events", dict(m.events), "flows", len(m.flows), "records", len(m.ps.table))
