"""AP by slice on the GPU (kitti_eval.evaluate_sliced).

1. Against the program: evaluate_object_3d_offline(_low_iou) from oracle/_ref/, run once per depth bin on the texts
   rewritten as tests/kitti_slice_cases.py defines a bin, against ONE evaluate_sliced call on the original texts with
   both IoU sets and the edges.  Every AP line and every detection-curve point must print equal; the orientation curves
   have the one-printed-unit allowance of test_kitti_eval_vs_program_gpu.py (the program sums in readdir order).
2. Against today's evaluator, to the bit: the 'all' slices against evaluate, every bin against evaluate on the
   rewritten frames (both sum in index order: no allowance), twice, and whatever other slices ride along.
3. Frame sizes around the bitset words, pre-filled buffers, the empty batch and the refusals.
4. The Evaluator's ap_slices on the fixture split."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_eval_cases as C  # noqa: E402
import kitti_program as P  # noqa: E402
import kitti_slice_cases as S  # noqa: E402
import mscnn_split  # noqa: E402

from monopsr_amd import _lib  # noqa: E402
from monopsr_amd.core import config_utils, evaluator, evaluator_utils  # noqa: E402
from monopsr_amd.core import kitti_eval as ke  # noqa: E402

pytestmark = pytest.mark.gpu

TALLY = P.CurveTally()
_FRAMES, _SLICED, _REWRITTEN, _RUNS = {}, {}, {}, {}


def _frames(name, iou):
    """The case's parsed frames in index order; `iou` picks the variant of strict_2d."""
    key = (name, iou if name == "strict_2d" else None)
    if key not in _FRAMES:
        gts, dets = S.by_index(S.case(name, iou))
        _FRAMES[key] = ([ke.parse_labels(t, False) for t in gts], [ke.parse_labels(t, True) for t in dets])
    return _FRAMES[key]


def _sliced(name, iou):
    """One evaluate_sliced call per case on the ORIGINAL texts: both IoU sets and the test edges, shared by the tests."""
    key = (name, iou if name == "strict_2d" else None)
    if key not in _SLICED:
        _SLICED[key] = ke.evaluate_sliced(*_frames(name, iou), ious=S.IOUS, depth_edges=S.EDGES)
    return _SLICED[key]


def _rewritten_frames(name, iou, lo, hi):
    key = (name, iou if name == "strict_2d" else None, lo, hi)
    if key not in _REWRITTEN:
        gts, dets = S.by_index(S.rewrite_case(S.case(name, iou), lo, hi))
        _REWRITTEN[key] = ([ke.parse_labels(t, False) for t in gts], [ke.parse_labels(t, True) for t in dets])
    return _REWRITTEN[key]


def _program(name, iou, label, tmp_path_factory):
    """The program's run on the case rewritten for a bin (run once in a session)."""
    key = (name, iou, label)
    if key not in _RUNS:
        lo, hi = S.BOUNDS[S.LABELS.index(label)]
        indices, gts, dets = S.rewrite_case(S.case(name, iou), lo, hi)
        _RUNS[key] = P.run_program(tmp_path_factory.mktemp("program"), indices, gts, dets, iou)
    return _RUNS[key]


def _curves(result):
    return {(c, k): v["curve"] for c, d in result.items() for k, v in d.items()}


def _equal(a, b):
    """Two results, to the bit: the same classes and keys, and every array equal with NaNs in the same places."""
    if set(a) != set(b):
        return False
    for cls in a:
        if set(a[cls]) != set(b[cls]):
            return False
        for key in a[cls]:
            for part in ("curve", "ap11", "ap40"):
                x, y = np.asarray(a[cls][key][part]), np.asarray(b[cls][key][part])
                if x.shape != y.shape or not np.array_equal(x, y, equal_nan=True):
                    return False
    return True


# ---------------------------------------------------------------------------------------------------- 1. the program

def test_the_edges_cut_cars_into_every_bin():
    for name in ("fixture", "classes", "synthetic_cut"):
        for lo, hi in S.BOUNDS:
            n_gt, n_det = S.in_bin_counts(S.case(name, "standard"), lo, hi)
            assert n_gt >= 1 and n_det >= 1, (name, lo, hi)


@pytest.mark.parametrize("iou", S.IOUS)
@pytest.mark.parametrize("name", S.NAMES)
def test_every_bin_matches_the_program_on_the_rewritten_texts(name, iou, tmp_path_factory):
    assert S.case(name, iou)[3] == 0
    results = _sliced(name, iou)
    assert list(results) == [(i, label) for i in S.IOUS for label in ("all",) + S.LABELS]
    for label in S.LABELS:
        run = _program(name, iou, label, tmp_path_factory)
        result = results[(iou, label)]
        lines = ke.format_report(result, None).splitlines() if result else []  # (no entry: the report is one '\n')
        assert lines == run.lines, (label, lines, run.lines)
        # a class for which the program prints no line has no entry
        assert set(result) == set(line.split("_")[0] for line in run.lines), label
        before = TALLY.allowance
        P.compare_curves(_curves(result), run, TALLY, allow_orientation_unit=True)
        TALLY.lines += len(lines)
        print("%s/%s/%s: %d AP lines equal, %d orientation points within one printed unit (running totals: %d lines, "
              "%d curve points, %d allowances)" % (name, iou, label, len(lines), TALLY.allowance - before, TALLY.lines,
                                                   TALLY.points, TALLY.allowance))


def test_the_program_prints_lines_in_most_runs(tmp_path_factory):
    """Equal empty outputs must not pass for agreement: at least 80 % of the (case, iou, bin) runs print an AP line."""
    runs = [_program(name, iou, label, tmp_path_factory) for name in S.NAMES for iou in S.IOUS for label in S.LABELS]
    with_lines = sum(1 for run in runs if run.lines)
    print("%d of %d runs of the program print AP lines" % (with_lines, len(runs)))
    assert len(runs) == len(S.NAMES) * 2 * 3 and with_lines >= 0.8 * len(runs)


# ---------------------------------------------------------------------------------------------------- 2. the evaluator

@pytest.mark.parametrize("name", S.NAMES)
def test_every_slice_is_evaluate_to_the_bit(name):
    gt, dets = _frames(name, "standard")
    results = _sliced(name, "standard")
    entries = 0
    for iou in S.IOUS:
        assert _equal(results[(iou, "all")], ke.evaluate(gt, dets, iou=iou)), (iou, "all")
        for label, (lo, hi) in zip(S.LABELS, S.BOUNDS):
            want = ke.evaluate(*_rewritten_frames(name, "standard", lo, hi), iou=iou)
            assert _equal(results[(iou, label)], want), (iou, label)
            entries += sum(len(d) for d in want.values())
    assert entries > 0
    assert all(_equal(a, b) for a, b in zip(results.values(), ke.evaluate_sliced(gt, dets, S.IOUS, S.EDGES).values()))


@pytest.mark.parametrize("name", ["fixture", "on_the_edges", "sizes"])
def test_a_slice_does_not_depend_on_the_slices_that_ride_along(name):
    """1, 6, 8 and 32 slices: 27, 162, 216 and 864 configurations, one to fourteen blocks of 64 lanes per frame."""
    gt, dets = _frames(name, "standard")
    eight = _sliced(name, "standard")
    one = ke.evaluate_sliced(gt, dets, ("low",), ())
    six = ke.evaluate_sliced(gt, dets, ("low", "standard"), (20.0,))
    edges = (20.0, 35.0) + tuple(36.0 + k for k in range(12))
    full = ke.evaluate_sliced(gt, dets, S.IOUS, edges)
    assert (len(one), len(six), len(full)) == (1, 6, 32)
    for iou in S.IOUS:
        assert _equal(full[(iou, "all")], eight[(iou, "all")]) and _equal(six[(iou, "all")], eight[(iou, "all")])
        assert _equal(full[(iou, "<20")], eight[(iou, "<20")]) and _equal(six[(iou, "<20")], eight[(iou, "<20")])
        assert _equal(full[(iou, "20-35")], eight[(iou, "20-35")])
    assert _equal(one[("low", "all")], eight[("low", "all")])
    # the last slice of the 32, a bin of its own: against evaluate on the rewritten frames
    lo = edges[-1]
    gts, dts = S.by_index(S.rewrite_case(S.case(name, "standard"), lo, np.inf))
    want = ke.evaluate([ke.parse_labels(t, False) for t in gts], [ke.parse_labels(t, True) for t in dts], iou="low")
    assert _equal(full[("low", ">=47")], want)


# ---------------------------------------------------------------------------------------------------- 3. sizes, refusals

def _size_texts():
    rng = np.random.default_rng(21)
    made = [C._crowd(rng, n, 6) for n in (0, 1, 32, 33, 65)]
    return ["\n".join(g) for g, _ in made], ["\n".join(d) for _, d in made]


def _parse(gts, dets):
    return [ke.parse_labels(t, False) for t in gts], [ke.parse_labels(t, True) for t in dets]


def _size_frames():
    return _parse(*_size_texts())


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_frame_sizes_on_prefilled_buffers(fill, monkeypatch):
    """Frames of 0, 1, 32, 33 and 65 detections; every buffer evaluate_sliced allocates holds the byte `fill` before
    the kernels write it.  The result is evaluate's, slice by slice, and the one-slice call is the old entry points'."""
    gt, dets = _size_frames()
    want = {(iou, "all"): ke.evaluate(gt, dets, iou=iou) for iou in S.IOUS}
    assert sum(len(d) for d in want[("low", "all")].values()) == 18  # 3 classes x (3 metrics + aos + 2 headings)
    empty = torch.empty

    def filled(*args, **kwargs):
        t = empty(*args, **kwargs)
        if t.is_cuda and t.numel():
            t.view(-1).view(torch.uint8).fill_(fill)
        return t
    monkeypatch.setattr(torch, "empty", filled)
    got = ke.evaluate_sliced(gt, dets, S.IOUS, S.EDGES)
    one = ke.evaluate_sliced(gt, dets, ("standard",), ())
    monkeypatch.undo()
    for iou in S.IOUS:
        assert _equal(got[(iou, "all")], want[(iou, "all")]), iou
    assert list(one) == [("standard", "all")] and _equal(one[("standard", "all")], want[("standard", "all")])
    gts, dts = _size_texts()
    for label, (lo, hi) in zip(S.LABELS, S.BOUNDS):
        in_bin = ke.evaluate(*_parse([S.rewrite_text(t, lo, hi, False) for t in gts],
                                     [S.rewrite_text(t, lo, hi, True) for t in dts]), iou="low")
        assert _equal(got[("low", label)], in_bin), label


def test_an_empty_batch():
    got = ke.evaluate_sliced([], [], S.IOUS, S.EDGES)
    assert len(got) == 8 and all(r == {} for r in got.values()) and ke.evaluate([], []) == {}
    # frames without a row
    none = [ke.parse_labels("", False)] * 3, [ke.parse_labels("", True)] * 3
    assert all(r == {} for r in ke.evaluate_sliced(none[0], none[1], S.IOUS, S.EDGES).values())


def test_refusals_with_a_real_batch():
    gt, dets = _size_frames()
    b = ke._Batch(gt, dets, None)
    lib, p = _lib.lib(), _lib.ptr
    host = (_lib.KittiSlice * 33)()
    for k in range(33):
        host[k].min_overlap[:] = [0.7, 0.5, 0.5] * 3
    dev = b.up(np.frombuffer(host, np.uint8), torch.uint8)
    overlaps = torch.zeros((6, b.n_pairs), dtype=torch.float64, device=b.dev)
    scores = torch.zeros((33 * 27, b.n_gt), dtype=torch.float64, device=b.dev)
    care = torch.zeros((33 * 27, b.nf), dtype=torch.int32, device=b.dev)

    def match(n, d=dev, h=host):
        return lib.mpsr_kitti_match_slices(ctypes.byref(b.struct), p(overlaps), None if d is None else p(d), h, n,
                                           p(scores), p(care), _lib.stream())
    assert match(33) == 1 and b"33 slices (1..32)" in lib.mpsr_last_error()
    assert match(0) == 1 and b"0 slices" in lib.mpsr_last_error()
    assert match(2, d=None) == 1 and b"slice table is null" in lib.mpsr_last_error()
    assert match(2, h=None) == 1 and b"slice table is null" in lib.mpsr_last_error()
    host[1].depth_tested, host[1].lo, host[1].hi = 1, 35.0, 20.0
    assert match(2) == 1 and b"hi < lo" in lib.mpsr_last_error()
    torch.cuda.synchronize()
    assert not scores.any() and not care.any()  # nothing was launched
    with pytest.raises(ValueError, match="at most 32"):
        ke.evaluate_sliced(gt, dets, S.IOUS, tuple(range(15)))


# ---------------------------------------------------------------------------------------------------- 4. the Evaluator

THRESHOLD, BATCH, STEP = 0.1, 2, 7


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    from monopsr_amd.datasets.kitti import kitti_dataset
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp("kitti_slices")))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, "test")
    ds = kitti_dataset.KittiDataset(dcfg, "val", mscnn_label_dir=mscnn)
    plain_out, out = str(tmp_path_factory.mktemp("plain")), str(tmp_path_factory.mktemp("sliced"))
    common = dict(batch_size=BATCH, iou="low")
    plain = evaluator.Evaluator(model, ds, THRESHOLD, predictions_base_dir=plain_out, **common).run_once(STEP)
    ev = evaluator.Evaluator(model, ds, THRESHOLD, predictions_base_dir=out, ap_slices=dict(depth_edges=(15.0, 30.0)),
                             **common)
    return dict(ds=ds, plain=plain, result=ev.run_once(STEP), out=out, plain_out=plain_out)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


def test_evaluator_slices_are_evaluate_sliced_on_its_frames(setup):
    ds, result = setup["ds"], setup["result"]
    names = sorted(ds.split_sample_names, key=lambda n: ke.frame_index(n + ".txt"))
    dets = [ke.parse_label_file(os.path.join(result["kitti_predictions_dir"], n + ".txt"), True) for n in names]
    gt = [ke.parse_label_file(os.path.join(ds.kitti_label_dir, n + ".txt"), False) for n in names]
    assert sum(len(d) for d in dets) == result["num_detections"] > 0
    want = ke.evaluate_sliced(gt, dets, ("standard", "low"), (15.0, 30.0))
    got = result["kitti_slices"]
    assert list(got) == list(want) == [(i, b) for i in ("standard", "low") for b in ("all", "<15", "15-30", ">=30")]
    assert all(_equal(got[k], want[k]) for k in want)
    assert _equal(got[("low", "all")], result["kitti"]) and sum(len(d) for d in result["kitti"].values()) > 0
    assert any(got[("low", label)] for label in ("<15", "15-30", ">=30"))


def test_evaluator_slice_files(setup):
    result, out = setup["result"], setup["out"]
    path = os.path.join(out, "kitti_reports", "val", "%08d_slices.txt" % STEP)
    assert result["kitti_slices_report"] == path
    with open(path) as f:
        assert f.read() == ke.format_sliced_report(result["kitti_slices"], STEP)
    csv_path = os.path.join(out, "metrics", "val", "ap_slices_val.csv")
    assert result["ap_slices_csv"] == csv_path
    with open(csv_path, newline="") as f:
        lines = f.read().split("\r\n")
    assert lines[-1] == "" and lines[0] == ",".join(evaluator_utils.AP_SLICES_HEADER)
    fields = [line.split(",") for line in lines[1:-1]]
    entries = [(iou, label, cls, key) for (iou, label), r in result["kitti_slices"].items() for cls, d in r.items()
               for key in d]
    assert [tuple(f[1:6]) for f in fields] == [e + (d,) for e in entries for d in ("easy", "moderate", "hard")]
    assert all(f[0] == "%d" % STEP and len(f) == 8 for f in fields)
    for f in fields:
        entry = result["kitti_slices"][(f[1], f[2])][f[3]][f[4]]
        d = ("easy", "moderate", "hard").index(f[5])
        for text, v in ((f[6], entry["ap11"][d]), (f[7], entry["ap40"][d])):
            assert text == ("nan" if v != v else "{:.5f}".format(v))


def test_evaluator_without_ap_slices_is_untouched(setup):
    plain, result = setup["plain"], setup["result"]
    new = {"kitti_slices", "kitti_slices_report", "ap_slices_csv"}
    assert set(result) - set(plain) == new and set(plain) <= set(result)
    for key in plain:
        if key.endswith("_csv") or key.endswith("_dir"):  # paths under the two output directories
            continue
        assert _same(plain[key], result[key]), key
    assert not os.path.exists(os.path.join(setup["plain_out"], "metrics", "val", "ap_slices_val.csv"))
    assert not os.path.exists(os.path.join(setup["plain_out"], "kitti_reports"))
