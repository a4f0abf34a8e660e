"""KITTI evaluation on the GPU (monopsr_amd.core.kitti_eval: evaluate, evaluate_dirs and the command line) against the
program itself: evaluate_object_3d_offline(_low_iou) compiled from the reference's unmodified sources against the
boost-free shim (oracle/ref_eval, built into oracle/_ref/ by build()), on the whole seeded catalogue of
kitti_eval_cases.py.  Every AP line must print equal, and every detection curve point.  The orientation curves may
differ by one printed unit (1e-6) where their strings differ, because the program sums the frames' similarities in
readdir order and the GPU evaluator in index order; the tests count how often that allowance was used."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_cases as C  # noqa: E402
import kitti_program as P  # noqa: E402

pytestmark = pytest.mark.gpu

TALLY = P.CurveTally()


def _ke():
    from monopsr_amd.core import kitti_eval as ke
    return ke


def _curves(result):
    return {(c, k): v["curve"] for c, d in result.items() for k, v in d.items()}


@pytest.mark.parametrize("iou", ["standard", "low"])
@pytest.mark.parametrize("name", C.NAMES)
def test_gpu_evaluator_matches_the_program(name, iou, tmp_path):
    ke = _ke()
    indices, gts, dets, dropped = C.case(name, iou)
    assert dropped == 0
    run = P.run_program(tmp_path, indices, gts, dets, iou)
    by_index = sorted(range(len(indices)), key=lambda k: indices[k])
    result = ke.evaluate([ke.parse_labels(gts[k], False) for k in by_index],
                         [ke.parse_labels(dets[k], True) for k in by_index], iou=iou)
    lines = ke.format_report(result, None).splitlines()
    assert lines == run.lines
    assert run.stats == P.expected_stats(lines, iou)
    before = TALLY.allowance
    P.compare_curves(_curves(result), run, TALLY, allow_orientation_unit=True)
    TALLY.lines += len(lines)
    print("%s/%s: %d AP lines equal, %d orientation points within one printed unit (running totals: %d lines, "
          "%d curve points, %d allowances)" % (name, iou, len(lines), TALLY.allowance - before, TALLY.lines,
                                               TALLY.points, TALLY.allowance))

    # the same frames from the program's own files, through evaluate_dirs and the command line
    res = os.path.join(str(tmp_path), "result_dir")
    from_dirs = ke.evaluate_dirs(os.path.join(str(tmp_path), "gt_dir"), res, iou=iou)
    assert ke.format_report(from_dirs, None).splitlines() == run.lines
    for key, curve in _curves(result).items():
        assert np.array_equal(_curves(from_dirs)[key], curve, equal_nan=True), key
    env = dict(os.environ)
    env["PYTHONPATH"] = P.ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "monopsr_amd.core.kitti_eval", "gt_dir", "result_dir"]
    if iou == "low":
        cmd.append("--low-iou")
    proc = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          universal_newlines=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    assert proc.stdout == run.stdout
