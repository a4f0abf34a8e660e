"""The restatement of KITTI's evaluator (test_kitti_eval.restated_evaluate, the checker of the GPU tests) against the
program itself: evaluate_object_3d_offline(_low_iou) compiled from the reference's unmodified sources against the
boost-free shim (oracle/ref_eval, built into oracle/_ref/ by build()), on the whole seeded catalogue of
kitti_eval_cases.py.  The restatement reads the frames in the program's readdir order, so even its orientation
similarity sums are added in the same order: every AP line and every curve must print equal.  CPU only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_cases as C  # noqa: E402
import kitti_program as P  # noqa: E402
import test_kitti_eval as R  # noqa: E402


@pytest.mark.parametrize("iou", ["standard", "low"])
@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_matches_the_program(name, iou, tmp_path):
    indices, gts, dets, dropped = C.case(name, iou)
    assert dropped == 0  # the guard took nothing from the catalogue
    run = P.run_program(tmp_path, indices, gts, dets, iou)
    assert sorted(run.order) == sorted(indices)
    pos = {idx: k for k, idx in enumerate(indices)}
    order = [pos[i] for i in run.order]
    curves, lines = R.restated_evaluate([gts[k] for k in order], [dets[k] for k in order], iou)
    assert lines == run.lines  # the same classes and metrics, every AP string equal ('-nan' included)
    assert run.stats == P.expected_stats(run.lines, iou)
    tally = P.CurveTally()
    P.compare_curves(curves, run, tally, allow_orientation_unit=False)
    print("%s/%s: %d AP lines, %d curve points equal" % (name, iou, len(lines), tally.points))


def test_catalogue_reaches_what_it_claims(tmp_path):
    """The cases exercise what their names say, on the program's own output."""
    def lines(name, iou="standard"):
        indices, gts, dets, _ = C.case(name, iou)
        return P.run_program(tmp_path / name, indices, gts, dets, iou).lines

    on = lines("classes")
    off = lines("classes_alpha_off")
    mix = lines("fixture", "low")
    big = lines("max_frame")
    assert any(s.startswith("car_orientation") for s in on)
    assert not any("orientation" in s for s in off) and len(off) == len(on) - 3  # car, pedestrian, cyclist
    assert any(s.startswith("cyclist_detection AP: 0.000000") for s in on)  # detections, no ground truth
    assert len(mix) == 18
    assert len(big) == 18
    _, _, dets, _ = C.case("max_frame", "standard")
    assert max(len(t.splitlines()) for t in dets) == C.MAX_FRAME
    _, _, dets, _ = C.case("sizes", "standard")
    assert [len(t.splitlines()) for t in dets][:len(C.SIZES)] == list(C.SIZES)
