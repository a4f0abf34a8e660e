"""KittiDataset on the GPU: samples against build_training_sample, the jittered duplicates, determinism, one training
step and the absence of device-to-host copies on the batch path."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jitter_restatement as jr
from monopsr_amd.core.config_utils import ConfigObj
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils as iu, kitti_dataset, obj_utils

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FIX = np.load(os.path.join(GOLDEN, 'instance_fixture.npz'))
# name in the split -> fixture frame; 000010 is frame 000006 again under another index of the split file.
# 000000 holds one Pedestrian and keeps no label.
SPLIT = (('000000', '000000'), ('000006', '000006'), ('000001', '000001'), ('000010', '000006'), ('000002', '000002'))
FILTER = dict(difficulty_str='all', box_2d_height=None, truncation=None, occlusion=None, depth_range=[5, 80])
KEPT = {'000006': [0, 1, 2, 3], '000001': [1], '000010': [0, 1, 2, 3], '000002': [1]}
TENSOR_KEYS = ('rgb_image', 'boxes_2d', 'boxes_2d_norm', 'cam_p', 'est_view_angs', 'class_indices', 'mean_lwh',
               'prop_cen_z_offset', 'boxes_3d', 'gt_alpha_bins', 'gt_alpha_regs', 'gt_alpha_valid_bins', 'gt_view_angs',
               'gt_inst_xyz_maps_local', 'gt_inst_xyz_maps_global', 'gt_valid_mask_maps')
EXTRA_KEYS = ('sample_name', 'num_objs', 'oversample_indices', 'jitter_trials')
MAPS = ('gt_inst_xyz_maps_local', 'gt_inst_xyz_maps_global', 'gt_valid_mask_maps')


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    """dataset_dir with train.txt and training/{label_2, calib, image_2, depth_2_multiscale,
    instance_2_depth_2_multiscale} from the fixture frames, a seeded synthetic RGB."""
    top = tmp_path_factory.mktemp('kitti')
    split = top / 'training'
    dirs = ('label_2', 'calib', 'image_2', 'depth_2_multiscale', 'instance_2_depth_2_multiscale')
    for d in dirs:
        (split / d).mkdir(parents=True)
    rng = np.random.default_rng(0)
    for name, f in SPLIT:
        depth = Image.open(os.path.join(GOLDEN, 'depth_%s.png' % f))
        (split / 'label_2' / (name + '.txt')).write_text(str(FIX['labels_%s' % f]))
        p2 = ' '.join('%.12e' % v for v in FIX['p2_%s' % f].reshape(-1))
        (split / 'calib' / (name + '.txt')).write_text(
            'P2: %s\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\n' % p2)
        w, h = depth.size
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(str(split / 'image_2' / (name + '.png')))
        depth.save(str(split / dirs[3] / (name + '.png')))
        Image.open(os.path.join(GOLDEN, 'instance_%s.png' % f)).save(str(split / dirs[4] / (name + '.png')))
    (top / 'train.txt').write_text(''.join(name + '\n' for name, _ in SPLIT))
    return str(top)


def _config(root, jitter, num_boxes=8, oversample=True, **over):
    cfg = dict(name='kitti', dataset_dir=root, data_split='train', data_split_dir='training', num_boxes=num_boxes,
               classes=['Car'], oversample=oversample, num_alpha_bins=12, alpha_bin_overlap=0.0,
               use_mscnn_detections=True, obj_filter_config=dict(FILTER),
               aug_config=dict(use_image_aug=False, box_jitter_type=jitter), depth_version='multiscale',
               instance_version='depth_2_multiscale')
    cfg.update(over)
    return ConfigObj(cfg)


def _dataset(root, jitter, mode='train', seed=0, **kw):
    return kitti_dataset.KittiDataset(_config(root, jitter, **kw), mode, seed=seed)


def _dirs(root):
    split = os.path.join(root, 'training')
    return split, os.path.join(split, 'depth_2_multiscale'), os.path.join(split, 'instance_2_depth_2_multiscale')


class _Choice:
    """A generator whose choice returns the sample's own oversampling draw."""

    def __init__(self, indices):
        self.indices = indices

    def choice(self, n, size, replace=True):
        assert len(self.indices) == size and (self.indices < n).all()
        return self.indices


def _host_sample(root, s, num_boxes):
    split, depth_dir, inst_dir = _dirs(root)
    idx = s['oversample_indices'].cpu().numpy().astype(np.int64)
    return kitti_dataset.build_training_sample(split, s['sample_name'], depth_dir, inst_dir, _Choice(idx[s['num_objs']:]),
                                               num_boxes=num_boxes, obj_filter=FILTER)


def _equal(a, b, keys=TENSOR_KEYS, rows=slice(None)):
    for k in keys:
        x, y = (a[k], b[k]) if k in ('rgb_image', 'cam_p') else (a[k][rows], b[k][rows])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        assert torch.equal(x, y), k


def _one_epoch(ds, batch_size, shuffle):
    """name -> the frame's sample of epoch 0 (its first occurrence), from next_batch."""
    seen = {}
    while len(seen) < ds.num_samples:
        batch = ds.next_batch(batch_size, shuffle)
        assert len(batch) == batch_size
        for s in batch:
            seen.setdefault(s['sample_name'], s)
    return seen


def test_dataset_without_jitter_equals_build_training_sample(root):
    ds = _dataset(root, None)
    assert ds.num_samples == 4 and ds.num_skipped == 1 and ds.sample_names == ['000006', '000001', '000010', '000002']
    assert ds.resident_bytes >= 2 * 8 * (375 * 1242 + 374 * 1238)
    samples = _one_epoch(ds, 3, shuffle=False)
    assert ds.epochs_completed == 1 and ds._index_in_epoch == 2
    for name, s in samples.items():
        assert set(s) == set(TENSOR_KEYS) | set(EXTRA_KEYS)
        assert s['num_objs'] == len(KEPT[name]) and s['oversample_indices'].dtype == torch.int32
        idx = s['oversample_indices'].cpu().numpy()
        assert list(idx[:s['num_objs']]) == list(range(s['num_objs'])) and idx.max() < s['num_objs']
        assert np.array_equal(idx, jr.oversample_indices(s['num_objs'], 8, [n for n, _ in SPLIT].index(name), 0, 0))
        assert (s['jitter_trials'] == 0).all()
        _equal(s, _host_sample(root, s, 8))
        assert float(s['gt_valid_mask_maps'].sum()) > 0
    assert ds.status() == (0, 0)
    ds.check_status()
    # 'val' never jitters; its samples are those of box_jitter_type None
    val = _dataset(root, 'oversample', mode='val', use_mscnn_detections=False)
    for s in val.get_sample_dict([0, 1, 2, 3]):
        _equal(s, samples[s['sample_name']])
    # oversample: False gives num_objs boxes
    plain = _dataset(root, 'all', oversample=False)
    for s in plain.next_batch(4, False):
        assert s['boxes_2d'].shape == (s['num_objs'], 4) and s['gt_valid_mask_maps'].shape == (s['num_objs'], 48, 48, 1)
        _equal(s, samples[s['sample_name']], keys=('boxes_3d', 'gt_alpha_bins', 'rgb_image'), rows=slice(0, s['num_objs']))
        assert (s['jitter_trials'] >= 1).all()
    assert plain.status() == (0, 0)


def _check_jittered_slots(root, s, base, rows):
    """The slots `rows` of sample s hold a jittered 2-D box of the label they duplicate and that label's other rows."""
    split, _, _ = _dirs(root)
    kept, _ = kitti_dataset.training_labels(split, s['sample_name'], ['Car'], FILTER)
    idx = s['oversample_indices'].cpu().numpy()
    for k in ('boxes_3d', 'gt_alpha_bins', 'gt_alpha_regs', 'gt_alpha_valid_bins', 'gt_view_angs', 'class_indices',
              'mean_lwh', 'prop_cen_z_offset'):
        assert torch.equal(s[k][rows], base[k][torch.as_tensor(idx, dtype=torch.long, device=base[k].device)][rows]), k
    h, w = s['rgb_image'].shape[0:2]
    label = np.array([[float(o.x1), float(o.y1), float(o.x2), float(o.y2)] for o in kept[idx]])
    b = s['boxes_2d'].cpu().numpy()
    trials = s['jitter_trials'].cpu().numpy()
    big = (label[:, 2] - label[:, 0] >= 10) & (label[:, 3] - label[:, 1] >= 10)
    assert big[rows].all() and (trials[rows] >= 1).all() and (trials <= 4096).all()
    got = b[:, [1, 0, 3, 2]].astype(np.float64)
    # the sample holds the box rounded to float32: each of the 4 edges moves by d <= 2^-15 px (half an ulp below 1024),
    # which moves the intersection and the union by at most d * max(w, h) each, so the IoU by at most
    # 8 d / min(w, h) <= 8 * 2^-15 / 10 = 2.5e-5 for a box of at least 10 px
    assert (jr.two_d_iou_pairs(got, label)[rows] >= 0.7 - 2.5e-5).all()
    assert (got[rows] != label[rows]).any(1).all()
    assert got[:, 0].min() >= 0 and got[:, 1].min() >= 0 and got[:, 2].max() <= w - 1 and got[:, 3].max() <= h - 1
    norm = (b.astype(np.float64) / np.array([h, w, h, w], np.float64)).astype(np.float32)
    assert s['boxes_2d_norm'].cpu().numpy().tobytes() == norm.tobytes()
    cam_p = s['cam_p'].cpu().numpy()
    p2 = FIX['p2_%s' % dict(SPLIT)[s['sample_name']]]
    assert np.array_equal(cam_p, p2.astype(np.float32))
    view = np.array([obj_utils.get_viewing_angle_box_2d(x, p2) for x in b], np.float32)
    gv = s['est_view_angs'].cpu().numpy()
    assert (np.abs(gv.astype(np.float64) - view) <= np.spacing(np.abs(view))).all()


def _check_maps(root, s):
    """The three ground-truth maps are instance_xyz_crops of the sample's own boxes, angles and ids."""
    split, depth_dir, inst_dir = _dirs(root)
    name = s['sample_name']
    _, ids = kitti_dataset.training_labels(split, name, ['Car'], FILTER)
    depth = depth_map_utils.read_depth_map(os.path.join(depth_dir, name + '.png'))
    inst = iu.read_instance_image(os.path.join(inst_dir, name + '.png'))
    n = s['boxes_2d'].shape[0]
    want = iu.instance_xyz_crops(depth[None], inst[None], s['cam_p'][None], np.zeros(n, np.int32),
                                 ids[s['oversample_indices'].cpu().numpy()], s['boxes_2d'], s['boxes_3d'],
                                 s['est_view_angs'])
    for a, k in zip(want, MAPS):
        assert torch.equal(a, s[k]), k


def test_dataset_with_oversample_jitter(root):
    base = {s['sample_name']: s for s in _dataset(root, None).get_sample_dict([0, 1, 2, 3])}
    ds = _dataset(root, 'oversample')
    samples = _one_epoch(ds, 4, shuffle=True)
    distinct = 0
    for name, s in samples.items():
        no = s['num_objs']
        b = base[name]
        assert torch.equal(s['oversample_indices'], b['oversample_indices'])
        # the labels themselves: the host's rows, bit for bit
        _equal(s, b, keys=[k for k in TENSOR_KEYS if k not in MAPS], rows=slice(0, no))
        _equal(s, _host_sample(root, s, 8), rows=slice(0, no))
        assert (s['jitter_trials'][:no] == 0).all()
        _check_jittered_slots(root, s, b, slice(no, 8))
        _check_maps(root, s)
        idx = s['oversample_indices'].cpu().numpy()[no:]
        dup = s['boxes_2d'].cpu().numpy()[no:]
        distinct = max(distinct, max(len(np.unique(dup[idx == k], axis=0)) for k in set(idx)))
    assert distinct >= 2
    assert ds.status() == (0, 0)
    ds.check_status()


def test_dataset_with_all_jitter(root):
    base = {s['sample_name']: s for s in _dataset(root, None).get_sample_dict([0, 1, 2, 3])}
    ds = _dataset(root, 'all')
    for s in ds.next_batch(4, False):
        assert torch.equal(s['oversample_indices'], base[s['sample_name']]['oversample_indices'])
        _check_jittered_slots(root, s, base[s['sample_name']], slice(0, 8))  # every box of the fixture is >= 10 px
        _check_maps(root, s)
    assert ds.status() == (0, 0)


def test_status_word_reports_a_bad_box(root):
    """The device-checked crop launch writes zeros for a box it rejects and says so."""
    from monopsr_amd import _lib
    depth = torch.rand((1, 20, 30), device='cuda') + 1
    inst = torch.zeros((1, 20, 30), dtype=torch.uint8, device='cuda')
    p2 = torch.tensor([[700.0, 0, 15, 40], [0, 700, 10, 0], [0, 0, 1, 0]], device='cuda').reshape(1, 12)
    b2 = torch.tensor([[2.0, 2, 10, 10], [3, 3, 3.4, 9], [3, 3, 9, 30.6], [0, 0, 5, float('nan')], [1, 1, 8, 8],
                       [1, 1, 8, 8]], device='cuda')
    fi = torch.tensor([0, 0, 0, 0, 1, 0], dtype=torch.int32, device='cuda')
    ids = torch.tensor([0, 0, 0, 0, 0, 255], dtype=torch.int32, device='cuda')
    b3 = torch.ones((6, 7), device='cuda')
    va = torch.zeros(6, device='cuda')
    out = [torch.full((6, 4, 4, c), float('nan'), device='cuda') for c in (3, 3, 1)]
    status = torch.zeros(2, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().mpsr_instance_xyz_crops_status(
        _lib.ptr(depth), _lib.ptr(inst), _lib.ptr(p2), 1, 20, 30, _lib.ptr(fi), _lib.ptr(ids), _lib.ptr(b2),
        _lib.ptr(b3), _lib.ptr(va), 6, 4, 4, 1, 1, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
        _lib.ptr(status), _lib.stream()))
    assert status.cpu().tolist() == [1 | 2 | 4 | 8, 5]
    for t in out:
        assert not torch.isnan(t).any() and (t[1:] == 0).all()
    want = iu.instance_xyz_crops(depth, inst, p2.reshape(1, 3, 4), fi[:1], ids[:1], b2[:1], b3[:1], va[:1], (4, 4))
    for a, b in zip(want, out):
        assert torch.equal(a[0], b[0])


def test_a_frames_sample_depends_on_seed_epoch_and_frame_only(root):
    ref = _one_epoch(_dataset(root, 'oversample', seed=3), 1, shuffle=False)
    for batch_size in (1, 3, 4):
        for shuffle in (False, True):
            got = _one_epoch(_dataset(root, 'oversample', seed=3), batch_size, shuffle)
            assert set(got) == set(ref)
            for name in ref:
                _equal(got[name], ref[name])
                assert torch.equal(got[name]['jitter_trials'], ref[name]['jitter_trials'])
    ds = _dataset(root, 'oversample', seed=3)
    names = ds.sample_names
    for s in ds.get_sample_dict([3, 1], epoch=0):
        _equal(s, ref[s['sample_name']])
    assert [s['sample_name'] for s in ds.get_sample_dict([3, 1])] == [names[3], names[1]]
    assert ds.epochs_completed == 0 and ds._index_in_epoch == 0
    # the two copies of one frame differ by their index in the split file alone
    assert not torch.equal(ref['000006']['boxes_2d'], ref['000010']['boxes_2d'])
    assert torch.equal(ref['000006']['boxes_2d'][:4], ref['000010']['boxes_2d'][:4])
    # other epochs and other seeds give other boxes
    e1 = {s['sample_name']: s for s in ds.get_sample_dict([0, 1, 2, 3], epoch=1)}
    other = {s['sample_name']: s for s in _dataset(root, 'oversample', seed=4).get_sample_dict([0, 1, 2, 3], epoch=0)}
    for name in ref:
        no = ref[name]['num_objs']
        for alt in (e1, other):
            assert not torch.equal(alt[name]['boxes_2d'][no:], ref[name]['boxes_2d'][no:])
            assert torch.equal(alt[name]['boxes_2d'][:no], ref[name]['boxes_2d'][:no])
    # the second pass of next_batch is epoch 1
    second = _dataset(root, 'oversample', seed=3)
    _one_epoch(second, 4, False)
    for s in second.next_batch(4, False):
        _equal(s, e1[s['sample_name']])


def test_one_trainer_step_on_a_jittered_sample(root):
    from monopsr_amd.core import config_utils, train_net, trainer
    from monopsr_amd.core import weights as W
    jit = {s['sample_name']: s for s in _dataset(root, 'oversample').get_sample_dict([0, 1, 2, 3])}['000006']
    plain = {s['sample_name']: s for s in _dataset(root, None).get_sample_dict([0, 1, 2, 3])}['000006']
    cfg = config_utils.default_config()
    weights = W.synthetic_weights(seed=111, width_div=8, scopes=(W.CROP_SCOPE, W.FULL_SCOPE))
    net = train_net.TrainNet(weights, width_div=8, full_trunk=True)
    tr = trainer.InstanceTrainer(net, cfg.model_config, cfg.dataset_config, lr=1e-4)
    with torch.no_grad():
        _, a = tr.loss(tr.forward(jit), jit)
        _, b = tr.loss(tr.forward(plain), plain)
    loss = float(tr.step(jit))
    assert np.isfinite(loss) and np.isfinite(float(a)) and np.isfinite(float(b))
    assert float(a) != float(b)


def _is_dtoh(name):
    n = name.lower().replace(' ', '').replace('_', '')
    return 'dtoh' in n or 'devicetohost' in n or 'device->host' in n or 'device->pageable' in n or 'device->pinned' in n


def test_next_batch_makes_no_device_to_host_copy(root):
    from torch.profiler import ProfilerActivity, profile
    ds = _dataset(root, 'oversample')
    for _ in range(3):
        ds.next_batch(3, True)
    torch.cuda.synchronize()
    # (1) torch refuses every synchronising call of its own while this mode is on
    torch.cuda.set_sync_debug_mode('error')
    try:
        for _ in range(3):
            ds.next_batch(3, True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    # (2) the profiler sees no device-to-host copy; a control run shows that it would
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as control:
        torch.ones(64, device='cuda').cpu()
        torch.cuda.synchronize()
    assert any(_is_dtoh(e.name) for e in control.events()), sorted({e.name for e in control.events()})
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(4):
            batch = ds.next_batch(3, True)
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events()})
    assert not [n for n in names if _is_dtoh(n)], names
    assert any('jitter_boxes_kernel' in n for n in names) and any('instance_crop_kernel' in n for n in names), names
    assert len(batch) == 3 and ds.status() == (0, 0)
