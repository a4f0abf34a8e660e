"""Scoring a reconstruction against ground truth without a GPU: the restatement against its own per-box loop, the
properties the catalogue is built for, the C entry point's host-side argument checks, the metric table's arithmetic, the
Evaluator's argument and the command line's flag."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import scene_restatement
import scene_score_cases as cases
import scene_score_restatement as restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('mpsr_scene_score_scratch_bytes', 'mpsr_scene_score')


@pytest.mark.parametrize('name', cases.NAMES)
def test_vectorised_restatement_equals_its_loop(name):
    want = restatement.scores_loop(cases.case(name), cases.ground_truth(name), cases.scene(name))
    got = cases.expected(name)
    assert got['counts'].shape == want['counts'].shape and np.array_equal(got['counts'], want['counts'])
    if name in cases.EXACT_NAMES:
        assert got['sums'].tobytes() == want['sums'].tobytes()
    else:
        bound = restatement.sum_bounds(cases.case(name), cases.ground_truth(name), cases.scene(name))
        assert bool((np.abs(got['sums'] - want['sums']) <= bound).all())
    c = got['counts']
    scene = cases.scene(name)
    assert np.array_equal(c[:, 0], scene['kept_per_box']) and np.array_equal(c[:, 2], scene['visible_per_box'])
    assert bool((c[:, 1] <= c[:, 0]).all() and (c[:, 3] <= c[:, 2]).all() and (c[:, 3] <= c[:, 4]).all())
    assert bool((c[:, 5] <= c[:, 3]).all() and (c[:, 3] <= c[:, 1]).all() and (c[:, 2] <= c[:, 0]).all())


@pytest.mark.parametrize('name', cases.EXACT_NAMES)
def test_exact_cases_lie_on_their_grids(name):
    """What makes the fp64 sums independent of their order: z of every kept point on the 2^-10 grid below 128 m, every
    finite ground-truth depth on the 2^-8 grid below 128 m, at most 2304 points in a box."""
    case, gt = cases.case(name), cases.ground_truth(name)
    z = np.asarray(case['xyz'], np.float32)[..., 2][scene_restatement.project(case) >= 0].astype(np.float64)
    assert bool((z > 0).all() and (z < cases.LIMIT).all()) and np.array_equal(np.rint(z / cases.Z_GRID) * cases.Z_GRID, z)
    for d in gt['depth_maps']:
        d = np.asarray(d, np.float64)
        d = d[np.isfinite(d)]
        assert bool((np.abs(d) < cases.LIMIT).all()) and np.array_equal(np.rint(d / cases.DEPTH_GRID) * cases.DEPTH_GRID, d)
    assert np.asarray(case['xyz']).shape[1] <= 2304
    # the largest sum of squares, in units of 2^-20, is an integer below 2^53
    s2 = cases.expected(name)['sums'][:, 2] * 2.0 ** 20
    assert np.array_equal(np.rint(s2), s2) and float(s2.max(initial=0.0)) < 2.0 ** 53


def test_the_catalogue_holds_what_it_is_meant_to_hold():
    sizes = {(np.asarray(cases.case(n)['xyz']).shape[0], np.asarray(cases.case(n)['xyz']).shape[1]) for n in cases.NAMES}
    assert {p for _, p in sizes} >= {1, 35, 64, 65, 300, 2304} and {b for b, _ in sizes} >= {1, 3, 70, 255}
    for name in ('grid_b70_p300', 'random_b70_p300'):
        gt, c = cases.ground_truth(name), cases.expected(name)['counts']
        gid, bf = gt['box_gt_id'], np.asarray(cases.case(name)['box_frame'])
        assert gid[3] == -1 and gid[4] == 300 and c[3, 1] == c[3, 3] == c[3, 4] == 0 and c[4, 4] == 0
        assert 0 <= gid[5] <= 254 and not (gt['instance_images'][bf[5]] == gid[5]).any() and c[5, 4] == 0
        assert gid[6] == gid[7] and bf[6] == bf[7] and c[6, 4] == c[7, 4] > 0
        assert len(gt['instance_images']) == 3 and [im.shape for im in gt['instance_images']] == [(5, 7), (8, 8), (6, 13)]
        assert int(c[:, 3].sum()) > 20 and int(c[:, 5].sum()) > 10 and int((c[:, 5] < c[:, 3]).sum()) > 0
        assert int((c[:, 1] > c[:, 3]).sum()) > 0          # points on the instance that lose their pixel
    for gt in (cases.ground_truth(n) for n in cases.NAMES):
        for im, d in zip(gt['instance_images'], gt['depth_maps']):
            assert im.dtype == np.uint8 and d.dtype == np.float32 and im.shape == d.shape
    d = np.concatenate([d.reshape(-1) for d in cases.ground_truth('random_b70_p300')['depth_maps']])
    assert bool((d == 0).any() and np.isinf(d).any() and np.isnan(d).any())
    assert cases.expected('boxes_255')['counts'].shape == (255, 6)


def test_identity_and_scaled_cases():
    """identity: every point on its own pixel of its own instance at the LiDAR's depth: inter = pred = gt pixels, the
    three sums exactly 0, IoU exactly 1.  scaled: the same pixels, 1.25 times as far: sum e = 0.25 sum d exactly."""
    ident, scaled = cases.expected('identity'), cases.expected('scaled')
    gt = cases.ground_truth('identity')
    px = np.asarray([24, 20])
    for got in (ident, scaled):
        c = got['counts']
        assert np.array_equal(c, np.stack([px] * 6, 1))
    assert not ident['sums'].any()
    table = restatement.table(ident['counts'], ident['sums'], gt['box_gt_id'])
    assert np.array_equal(table, np.asarray([[1, 1, 1, 0, 0, 0]] * 2, np.float32))
    d = gt['depth_maps'][0].astype(np.float64)
    for b, v in enumerate(gt['box_gt_id']):
        mine = d[gt['instance_images'][0] == v]
        assert scaled['sums'][b, 0] == 0.25 * mine.sum() == scaled['sums'][b, 1]
        assert scaled['sums'][b, 2] == (mine * mine).sum() / 16.0
    assert np.array_equal(restatement.table(scaled['counts'], scaled['sums'], gt['box_gt_id'])[:, :3], table[:, :3])
    assert np.array_equal(scene_restatement.project(cases.case('identity')), scene_restatement.project(cases.case('scaled')))
    # the same with a whole box of 2304 points
    big, gt = cases.expected('scaled_2304'), cases.ground_truth('scaled_2304')
    assert np.array_equal(big['counts'], np.stack([[2304, 400]] * 6, 1))
    assert np.array_equal(cases.expected('identity_2304')['counts'], big['counts'])
    assert not cases.expected('identity_2304')['sums'].any()
    mine = gt['depth_maps'][0].astype(np.float64)[gt['instance_images'][0] == 254]
    assert len(mine) == 2304 and big['sums'][0, 0] == 0.25 * mine.sum() and big['sums'][0, 2] == (mine * mine).sum() / 16.0


def test_new_names_are_declared_and_bound():
    from monopsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
        assert re.search(r'\b%s\s*\(' % name, header), name
    assert _lib.ABI_VERSION == 13 and _lib.lib().mpsr_abi_version() == 13
    assert len(_lib.SIGNATURES['mpsr_scene_score'][1]) == 18
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^[^\n#]*\bscene\.o\b[^\n]*:[^\n]*\n\t[^\n]*\$\(NOFMA\)', mk, re.M)


def _score(lib, nf, tp, nb, npts, ptr=None, bf=None, ws=(None, 0), scratch=(None, 0), **null):
    """mpsr_scene_score with `ptr` for every pointer (never dereferenced: each call fails or returns on the host)."""
    a = dict(xyz=ptr, box_frame=ptr, box_frame_host=ptr if bf is None else bf, gt_id=ptr, depth=ptr, inst=ptr, offs=ptr,
             counts=ptr, sums=ptr)
    a.update(null)
    return lib.mpsr_scene_score(a['xyz'], a['box_frame'], a['box_frame_host'], a['gt_id'], a['depth'], a['inst'],
                                a['offs'], nf, tp, nb, npts, ws[0], ws[1], scratch[0], scratch[1], a['counts'],
                                a['sums'], None)


def test_entry_point_checks_its_arguments_without_a_gpu():
    from monopsr_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(256)
    host = lambda values: np.ascontiguousarray(np.asarray(values, np.int32))
    as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # the scratch size helper: 256 int32 per frame
    sb = lib.mpsr_scene_score_scratch_bytes
    assert sb(0) == 0 and sb(-3) == 0 and sb(1) == 1024 and sb(8) == 8192
    # empty sizes: no-ops, whatever the pointers
    for nf, tp, nb, npts in ((0, 10, 3, 4), (2, 10, 0, 4), (2, 10, 3, 0), (0, 0, 0, 0), (2, 0, 3, 4)):
        assert _score(lib, nf, tp, nb, npts) == 0
    # negative sizes
    for nf, tp, nb, npts in ((-1, 10, 3, 4), (2, -10, 3, 4), (2, 10, -3, 4), (2, 10, 3, -4)):
        assert _score(lib, nf, tp, nb, npts) == 1 and b'negative' in lib.mpsr_last_error()
    # null pointers with non-empty sizes: all of them, and each one alone
    assert _score(lib, 2, 10, 3, 4) == 1 and b'null' in lib.mpsr_last_error()
    bf = host([0, 1, 1])
    for key in ('xyz', 'box_frame', 'box_frame_host', 'gt_id', 'depth', 'inst', 'offs', 'counts', 'sums'):
        assert _score(lib, 2, 99, 3, 4, fake, as_ptr(bf), **{key: None}) == 1, key
        assert b'null' in lib.mpsr_last_error(), key
    # the point index must fit the key's 32 bits
    assert _score(lib, 1, 10, 65536, 65536) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert _score(lib, 1, 10, 65535, 65536) == 1 and b'null' in lib.mpsr_last_error()  # past that check
    # box_frame_host: in range and never decreasing
    for bad, what in (([0, 2, 1], b'of frame 2'), ([1, 0, 1], b'decreases'), ([0, -1, 1], b'of frame -1')):
        b = host(bad)
        assert _score(lib, 2, 99, 3, 4, fake, as_ptr(b)) == 1 and what in lib.mpsr_last_error()
    # the workspace, then the scratch: status 3, still before any launch
    assert _score(lib, 2, 99, 3, 4, fake, as_ptr(bf)) == 3 and b'workspace' in lib.mpsr_last_error()
    need = lib.mpsr_scene_workspace_bytes(2, 99, 3, 4)
    assert _score(lib, 2, 99, 3, 4, fake, as_ptr(bf), ws=(fake, need - 1)) == 3 and b'workspace' in lib.mpsr_last_error()
    assert _score(lib, 2, 99, 3, 4, fake, as_ptr(bf), ws=(fake, need)) == 3 and b'scratch' in lib.mpsr_last_error()
    assert _score(lib, 2, 99, 3, 4, fake, as_ptr(bf), ws=(fake, need), scratch=(fake, 2 * 1024 - 1)) == 3
    assert b'scratch' in lib.mpsr_last_error()
    assert _score(lib, 2, 99, 3, 4, fake, as_ptr(bf), ws=(fake, need), scratch=(None, 2 * 1024)) == 3


def test_table_arithmetic_and_nan_rules():
    """score_table on hand-made counts (CPU tensors): fp64 quotients rounded once, NaN exactly where there is none."""
    import torch
    from monopsr_amd.core import scene_reconstruction as sr
    assert sr.SCENE_METRIC_NAMES == restatement.METRIC_NAMES and sr.SCENE_COUNT_NAMES == restatement.COUNT_NAMES
    #          kept on pred inter gt depth_n
    counts = [[10, 6, 8, 4, 12, 3],      # everything defined: IoU 4 / 16
              [10, 0, 8, 0, 0, 0],       # no ground truth (-1): IoU NaN although pred > 0
              [0, 0, 0, 0, 5, 0],        # nothing kept: IoU 0 / 5 = 0, both precisions NaN
              [7, 0, 0, 0, 0, 0],        # kept but never visible, an id no pixel has: union 0 -> NaN; point precision 0
              [3, 3, 3, 3, 3, 0],        # a perfect mask without a measured depth
              [2304, 2303, 1, 1, 100000, 1],
              [9, 9, 9, 9, 9, 9]]        # id 300: no ground truth
    sums = [[0.75, 1.5, 3.0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [-0.1, 0.1, 0.1 * 0.1], [9.0, 9.0, 9.0]]
    gid = [0, -1, 254, 17, 3, 9, 300]
    got = sr.score_table(torch.tensor(counts, dtype=torch.int32), torch.tensor(sums, dtype=torch.float64),
                         torch.tensor(gid, dtype=torch.int32))
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 6)
    got = got.numpy()
    nan = np.nan
    want = np.asarray([[4 / 16, 4 / 8, 6 / 10, 0.25, 0.5, 1.0],
                       [nan, 0.0, 0.0, nan, nan, nan],
                       [0.0, nan, nan, nan, nan, nan],
                       [nan, nan, 0.0, nan, nan, nan],
                       [1.0, 1.0, 1.0, nan, nan, nan],
                       [1 / 100000, 1.0, 2303 / 2304, -0.1, 0.1, np.sqrt(0.1 * 0.1)],
                       [nan, 1.0, 1.0, 1.0, 1.0, 1.0]], np.float64).astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
    assert np.array_equal(np.nan_to_num(restatement.table(counts, sums, gid)), np.nan_to_num(want))
    scores = sr.SceneScores(torch.tensor(counts, dtype=torch.int32), torch.tensor(sums, dtype=torch.float64),
                            torch.tensor(gid, dtype=torch.int32))
    assert np.array_equal(np.nan_to_num(scores.table().numpy()), np.nan_to_num(want))
    assert 'scores' in sr.SceneResult.__slots__


def test_restated_statistics():
    v = np.asarray([[1.0, np.nan], [np.nan, np.nan], [-3.0, np.nan]], np.float32)
    s = restatement.stats(v)
    assert s[0].tolist() == [2.0, -1.0, 2.0, 2.0, 1.0] and s[1, 0] == 0 and bool(np.isnan(s[1, 1:]).all())


def test_scene_metrics_defaults_to_false():
    from monopsr_amd.core import evaluator
    from monopsr_amd.core import scene_reconstruction as sr
    sig = inspect.signature(evaluator.Evaluator.__init__)
    assert sig.parameters['scene_metrics'].default is False
    for fn in (sr.project_instance_points, sr.reconstruct_frames):
        assert inspect.signature(fn).parameters['ground_truth'].default is None


def test_run_evaluation_accepts_scene_metrics():
    from monopsr_amd.experiments import run_evaluation
    need = ['cfg.yaml', '--checkpoint-dir', 'c', '--mscnn-dir', 'm', '--predictions-dir', 'p']
    ap = run_evaluation.build_parser()
    assert ap.parse_args(need).scene_metrics is False
    assert ap.parse_args(need + ['--scene-metrics']).scene_metrics is True
    stats = {n: dict(count=3, mean=0.5, std=0.25, mean_abs=0.5, std_abs=0.25, dropped=1) for n in restatement.METRIC_NAMES}
    text = run_evaluation.format_result(dict(report='R\n', scene_stats=stats))
    lines = text.splitlines()
    assert lines[0] == 'R' and [l.split()[0] for l in lines[1:]] == list(restatement.METRIC_NAMES)
    assert run_evaluation.format_result(dict(report='R\n')) == 'R\n'


def test_scene_stats_csv(tmp_path):
    from monopsr_amd.core import evaluator_utils
    names = restatement.METRIC_NAMES
    stats = {n: dict(count=k, mean=k + 0.5, std=0.125 * k, mean_abs=1.0, std_abs=0.0, dropped=0)
             for k, n in enumerate(names)}
    path = evaluator_utils.save_scene_stats(str(tmp_path), 'val', 40, names, stats)
    assert path == os.path.join(str(tmp_path), 'metrics', 'val', 'scene_metrics_val.csv')
    assert evaluator_utils.save_scene_stats(str(tmp_path), 'val', 80, names, stats) == path
    rows = [[c.strip() for c in line.split(',')] for line in open(path).read().splitlines()]
    assert len(rows) == 3 and all(len(r) == 1 + 3 * len(names) for r in rows)
    assert rows[0][:4] == ['step', 'mask_iou_count', 'mask_iou_mean', 'mask_iou_std'] and rows[0][-1] == 'depth_rmse_std'
    assert rows[1][0] == '40' and rows[2][0] == '80' and rows[1][1:] == rows[2][1:]
    assert rows[1][4:7] == ['1', '1.50000', '0.12500']
