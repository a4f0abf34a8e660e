"""Runs KITTI's native evaluator -- evaluate_object_3d_offline(_low_iou), compiled from the reference's unmodified
sources against the boost-free shim of oracle/ref_eval/ into oracle/_ref/ by build() -- on label texts, and parses
what it leaves: the '... AP: e m h' lines of its stdout, the 41-point curves of its plot directory (as printed, %f)
and the stats_*.txt files it chose to write.  A test helper, not a conftest: the differential tests import it."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
PROGRAMS = {"standard": "evaluate_object_3d_offline", "low": "evaluate_object_3d_offline_low_iou"}
SHIM_PROBE = os.path.join(REF_BIN, "shim_probe")


def binary(name):
    """The path of a binary build() made under oracle/_ref/.  A missing one is a failure, never a skip."""
    path = os.path.join(REF_BIN, name)
    assert os.access(path, os.X_OK), "%s is missing: build() compiles it (oracle/ref_eval/Makefile)" % path
    return path


class ProgramRun(object):
    """stdout: the program's stdout; lines: its AP lines; curves: {plot file stem: (41, 3) array of the printed
    strings of columns 2-4 (easy, moderate, hard)}; stats: the set of stats_*.txt names; order: the frame indices in
    the order the program read them (readdir order of result_dir/data)."""

    def __init__(self, stdout, lines, curves, stats, order):
        self.stdout, self.lines, self.curves, self.stats, self.order = stdout, lines, curves, stats, order


def write_inputs(tmp_path, indices, gt_texts, det_texts):
    """gt_dir/%06d.txt and result_dir/data/%06d.txt under tmp_path, one pair per frame index."""
    gt_dir = os.path.join(str(tmp_path), "gt_dir")
    data = os.path.join(str(tmp_path), "result_dir", "data")
    os.makedirs(gt_dir)
    os.makedirs(data)
    for idx, g, d in zip(indices, gt_texts, det_texts):
        with open(os.path.join(gt_dir, "%06d.txt" % idx), "w") as f:
            f.write(g + ("\n" if g else ""))
        with open(os.path.join(data, "%06d.txt" % idx), "w") as f:
            f.write(d + ("\n" if d else ""))
    return gt_dir, os.path.dirname(data)


def run_program(tmp_path, indices, gt_texts, det_texts, iou, timeout=300):
    """Writes the frames and runs the program in tmp_path as `<program> gt_dir result_dir` (relative names: the
    program prints no step line).  gnuplot's 'not found' on stderr is expected; anything the program reports on
    stdout that is not an AP line fails."""
    exe = binary(PROGRAMS[iou])
    write_inputs(tmp_path, indices, gt_texts, det_texts)
    proc = subprocess.run([exe, "gt_dir", "result_dir"], cwd=str(tmp_path), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    lines = proc.stdout.splitlines()
    assert all(" AP: " in line for line in lines), proc.stdout  # 'ERROR: Couldn't read ...' and the like
    res = os.path.join(str(tmp_path), "result_dir")
    plot = os.path.join(res, "plot" if iou == "standard" else "plot_low_iou")
    curves = {}
    for name in sorted(os.listdir(plot)):
        if not name.endswith(".txt"):
            continue
        with open(os.path.join(plot, name)) as f:
            rows = [line.split() for line in f.read().splitlines() if line.strip()]
        assert len(rows) == 41 and all(len(r) == 4 for r in rows), name
        curves[name[:-4]] = np.array([r[1:] for r in rows])
    stats = set(n for n in os.listdir(res) if n.startswith("stats_"))
    order = [_atoi(n[-10:]) for n in os.listdir(os.path.join(res, "data")) if len(n) >= 10]
    return ProgramRun(proc.stdout, lines, curves, stats, order)


def _atoi(s):
    """C atoi, as getEvalIndices applies it to a file name's last 10 characters."""
    s = s.lstrip()
    k = 1 if s[:1] in "+-" else 0
    e = k
    while e < len(s) and s[e].isdigit():
        e += 1
    return int(s[:e]) if e > k else 0


def expected_stats(lines, iou):
    """The stats_*.txt names the program writes for the AP lines it printed (eval :911-956: the BEV and 3D passes
    share one name; only the image pass's names carry _low_iou)."""
    suffix = "" if iou == "standard" else "_low_iou"
    out = set()
    for line in lines:
        name = line.split(" AP:")[0]
        cls, kind = name.split("_", 1)
        if kind == "detection":
            out.add("stats_%s_detection%s.txt" % (cls, suffix))
        elif kind == "orientation":
            out.add("stats_%s_orientation%s.txt" % (cls, suffix))
        elif kind in ("detection_BEV", "detection_3D"):
            out.add("stats_%s_detection_ground.txt" % cls)
    return out


# The plot files hold the detection curves of every pass and the orientation curve of the image pass; the heading
# curves reach stdout only as AP lines.
CURVE_FILES = {"image": "%s_detection", "aos": "%s_orientation", "bev": "%s_detection_BEV", "3d": "%s_detection_3D"}


def printf_f(v):
    """glibc's printf("%f"): NaNs print with their sign ('-nan' for x86's default NaN of 0.0 / 0.0)."""
    v = float(v)
    if v != v:
        return "-nan" if np.signbit(v) else "nan"
    return "%f" % v


class CurveTally(object):
    """Counts what a comparison of curves covered: points compared, and points of orientation-similarity curves that
    differed in their printed string by at most one unit (1e-6) -- the allowance for a similarity summed in another
    frame order."""

    def __init__(self):
        self.points = 0
        self.allowance = 0
        self.lines = 0


def compare_curves(curves, run, tally, allow_orientation_unit):
    """curves: {(class, key): (3, 41) float array} against the program's plot files.  Detection curves must print
    equal; orientation ('aos') curves too, unless allow_orientation_unit, where a point whose string differs may
    differ by at most 1e-6 of the printed values."""
    expected = set()
    for (cls, key), curve in curves.items():
        if key not in CURVE_FILES:
            continue
        stem = CURVE_FILES[key] % cls
        expected.add(stem)
        assert stem in run.curves, "the program wrote no %s.txt" % stem
        got = np.array([[printf_f(v) for v in row] for row in np.asarray(curve).T])  # (41, 3)
        want = run.curves[stem]
        tally.points += want.size
        diff = got != want
        if not diff.any():
            continue
        assert key == "aos" and allow_orientation_unit, "%s: %d points print differently, first %s" % (
            stem, int(diff.sum()), [(int(i), int(j), got[i, j], want[i, j]) for i, j in zip(*np.nonzero(diff))][:3])
        for i, j in zip(*np.nonzero(diff)):
            assert "nan" not in got[i, j] and "nan" not in want[i, j], (stem, got[i, j], want[i, j])
            assert abs(float(got[i, j]) - float(want[i, j])) <= 1.0000001e-6, (stem, i, j, got[i, j], want[i, j])
            tally.allowance += 1
    assert expected == set(run.curves), (sorted(expected), sorted(run.curves))
