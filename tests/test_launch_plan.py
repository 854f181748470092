"""The host-only launch planner (csrc/launch_plan.cpp) on the CPU: ppe_plan_image reproduces, field by field, the
plans recorded in tests/golden/launch_plans_v1.npz from the engine as it was before the planner was split out of
its launch path (image placement, tile fetch, workgroup size, LDS offsets and every image-derived kernel argument),
and ppe_pick_groups the batch-group choices recorded the same way.

The fixture's matrix: synth.make_rules(n, seed=n) for n in SIZES, each built under the four builder environments of
BUILDS, plus a 1,024-rule set with unused slots (index table) and a 640-rule set with residual MAC / time records;
the default tuning, every entry of tests/test_gpu_parity.py's TUNINGS and pipeline 3 at block 256; stateless and
flow-table plans.  Every return path of the planner has rows, but for two that no buildable image reaches: a jump
table (node walk) or block jump table (multi-tile walk) larger than the workgroup's whole LDS share."""
import ctypes as C
import os
import zlib
from pathlib import Path

import numpy as np
import pytest

from ppe import abi, synth

GOLDEN = Path(__file__).resolve().parent / "golden"

SIZES = (0, 1, 256, 1024, 4096, 16384, 65536)
BUILDS = {"default": {}, "nocut": {"PPE_CUT": "0"}, "nocut_nocompact": {"PPE_CUT": "0", "PPE_COMPACT": "0"},
          "cutlines": {"PPE_CUT_LINES": "1"}}
BUILD_ENV = ("PPE_CUT", "PPE_COMPACT", "PPE_CUT_LINES", "PPE_CUT_BITS", "PPE_JUMP_BITS", "PPE_LEAF_CAP_DEPTH",
             "PPE_LEAF_CAP_N")  # every variable the image builder reads
TUNING_FIELDS = [name for name, _ in abi.Tuning._fields_]


def build_images():
    """(name, image words) of every rule set of the matrix, each built once."""
    saved = {k: os.environ.pop(k, None) for k in BUILD_ENV}
    try:
        for n in SIZES:
            rules = synth.make_rules(n, seed=n)
            for build, env in BUILDS.items():
                os.environ.update(env)
                try:
                    yield f"n{n}/{build}", abi.build_image(rules, default_action=1)[0]
                finally:
                    for k in env:
                        del os.environ[k]
        used = np.ones(1024, np.uint8)
        used[::7] = 0  # holes: rule slots != rule indices, so the image carries the slot -> index table
        yield "n1024/holes", abi.build_image(synth.make_rules(1024, seed=1024), used, default_action=1)[0]
        # MAC / time fields on a tenth of the rules: the image carries residual records, and node walks at 512 and
        # 1024 threads stage everything before them (the split plan no other set of the matrix reaches)
        yield "n640/resid", abi.build_image(synth.make_rules(640, seed=640, resid_frac=0.1), default_action=1)[0]
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def plan_image(img: np.ndarray, tuning: dict, flow: int) -> dict:
    img = np.ascontiguousarray(img, np.uint32)
    t, p = abi.Tuning(**tuning), abi.Plan()
    rc = abi.load().ppe_plan_image(img.ctypes.data, len(img), C.byref(t), flow, C.byref(p))
    assert rc == 0, f"ppe_plan_image: {rc}"
    return p.as_dict()


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "launch_plans_v1.npz")


@pytest.fixture(scope="module")
def images(fixture):
    """The matrix's images, rebuilt; a builder that drifted from the fixture's is reported as such."""
    imgs = dict(build_images())
    assert list(imgs) == list(fixture["images"])
    for name, nw, crc in zip(fixture["images"], fixture["image_n_words"], fixture["image_crc"]):
        img = imgs[str(name)]
        assert (len(img), zlib.crc32(img.tobytes())) == (int(nw), int(crc)), \
            f"{name}: the image builder's output changed (not a planner failure): re-record the fixture"
    return imgs


def test_plan_fields_are_the_fixture_columns(fixture):
    assert list(fixture["fields"]) == abi.PLAN_FIELDS
    assert list(fixture["tuning_fields"]) == TUNING_FIELDS
    assert C.sizeof(abi.Plan) == 4 * len(abi.PLAN_FIELDS)


def test_fixture_covers_the_parity_tunings(fixture):
    from test_gpu_parity import TUNINGS
    have = {tuple(int(x) for x in row) for row in fixture["tunings"]}
    for tune in [dict()] + TUNINGS + [dict(pipeline=3, block=256)]:
        t = abi.Tuning(**tune).as_dict()
        assert tuple(t[k] for k in TUNING_FIELDS) in have, tune


def test_planner_reproduces_recorded_plans(fixture, images):
    names = [str(x) for x in fixture["images"]]
    tunings = [dict(zip(TUNING_FIELDS, (int(x) for x in row))) for row in fixture["tunings"]]
    plans = fixture["plans"]
    assert len(plans) == len(names) * len(tunings) * 2
    bad = []
    for row, ii, ti, flow in zip(plans, fixture["case_image"], fixture["case_tuning"], fixture["case_flow"]):
        got = plan_image(images[names[ii]], tunings[ti], int(flow))
        for k, want in zip(abi.PLAN_FIELDS, row):
            if got[k] != int(want):
                bad.append(f"{names[ii]} {tunings[ti]} flow={int(flow)}: {k} = {got[k]}, recorded {int(want)}")
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:20])


def test_planner_rejects_what_is_no_image():
    lib, t, p = abi.load(), abi.Tuning(), abi.Plan()
    words = abi.build_image(synth.make_rules(16))[0]
    assert lib.ppe_plan_image(words.ctypes.data, len(words), C.byref(t), 0, C.byref(p)) == 0
    assert lib.ppe_plan_image(words.ctypes.data, 8, C.byref(t), 0, C.byref(p)) == abi.PPE_EINVAL
    broken = words.copy()
    broken[0] ^= 1  # the magic word
    assert lib.ppe_plan_image(broken.ctypes.data, len(broken), C.byref(t), 0, C.byref(p)) == abi.PPE_EINVAL
    t = abi.Tuning(block=100)
    assert lib.ppe_plan_image(words.ctypes.data, len(words), C.byref(t), 0, C.byref(p)) == abi.PPE_EINVAL


def test_pick_groups(fixture):
    lib = abi.load()
    got = [lib.ppe_pick_groups(nb, 8) for nb in range(1, 41)]
    assert got == [int(x) for x in fixture["groups_cap8"]]
    assert (got[20 - 1], got[32 - 1], lib.ppe_pick_groups(33, 8)) == (4, 8, 2)
    assert got[33 - 1] == 2
