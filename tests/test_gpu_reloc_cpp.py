"""examples/reloc_harness: Tracking::Relocalization in one call from compiled C++.  Its lld_amd.hpp route (TrackedFrame::ComputeBoW /
Relocalization / Download) gives the reference's record, and adapters/lld_tracking_adapter.cc's Relocalization leaves in the Frame /
MapPoint test doubles what the reference's routine leaves - return value, mvpMapPoints, mvbOutlier, mTcw - against tests/reloc_ref.py; on a
scene nothing matches it returns false with the objects untouched."""
import os
import subprocess

import numpy as np
import pytest

import bow_ref
import reloc_ref as RF
import reloc_scenes as RS2
from lld_slam_amd import tracking
from test_gpu_reloc import same_integers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "examples", "reloc_harness")
SCENES = ("keeps_outliers", "no_match")


@pytest.fixture(scope="module")
def ran(oracle, tmp_path_factory):
    out = {}
    for name in SCENES:
        S = RS2.make_scene(name); sc = S["sc"]
        d = tmp_path_factory.mktemp("reloc_" + name)
        bow_ref.write_text(S["vocab"], d / "voc.txt")
        tracking.write_reloc_scene(d / "in.bin", sc["frame"], sc["cam"], S["candidates"], S["seeds"], S["Tcw0"], S["levelsup"])
        p = subprocess.run([HARNESS, str(d / "voc.txt"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        out[name] = dict(S=S, got=tracking.read_reloc_result(d / "out.bin", sc["frame"].n, len(S["candidates"])), ref=RF.relocalize(S))
    return out


@pytest.mark.parametrize("name", SCENES)
def test_harness_record_is_the_reference(ran, name):
    g, e = ran[name]["got"], ran[name]["ref"]
    assert g["returned"] == e["matched"]
    same_integers(g["record"], e, name)
    np.testing.assert_array_equal(g["kp_point_id"], e["kp_point_id"]); np.testing.assert_array_equal(g["kp_outlier"], e["kp_outlier"])


def test_adapter_writes_back_what_the_reference_leaves(ran):
    r = ran["keeps_outliers"]; a = r["got"]["adapter"]; e = r["ref"]
    assert a["returned"] == 1 == e["matched"]
    np.testing.assert_array_equal(a["point_id"], e["kp_point_id"])
    np.testing.assert_array_equal(a["outlier"], e["kp_outlier"])
    assert a["outlier"].sum() >= 3                                           # the flagged points of the second PoseOptimization stay in the frame
    np.testing.assert_array_equal(a["Tcw"], r["got"]["record"]["Tcw"])
    np.testing.assert_allclose(a["Tcw"], e["Tcw"], rtol=0, atol=1e-5)


def test_adapter_returns_false_with_the_objects_untouched(ran):
    r = ran["no_match"]; a = r["got"]["adapter"]; S = r["S"]
    assert a["returned"] == 0 == r["ref"]["matched"]
    assert np.all(a["point_id"] == -1) and not a["outlier"].any()
    np.testing.assert_array_equal(a["Tcw"], np.asarray(S["Tcw0"], np.float32).reshape(4, 4))
