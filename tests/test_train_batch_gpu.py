"""InstanceTrainer.step_batch: one training step on several frames (MonoPSRModel.build_train_batch / loss_batch) against
the frames' own single-frame steps.  The invariant is the one of tests/test_sharded_training_step_gpu.py: a multi-frame
step is the AVERAGE of the frames' own reference steps, not one step on the pooled boxes.

Narrow net (width_div 8), both trunks; lr = 0 so that the parameters never move and one trainer serves every run.  Frames
are built like _sample(full_trunk=True) of the sharded test: seeded boxes, trainer.synthetic_ground_truth, and the three
distinct cameras of tests/golden/instance_fixture.npz."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIX = np.load(os.path.join(GOLDEN, 'instance_fixture.npz'))
CAMS = [FIX[k].astype(np.float32) for k in ('p2_000000', 'p2_000001', 'p2_000006')]
DIV = 8
# (b) / (c): image size, camera, boxes per frame
FRAMES = (((375, 1242), 0, 2), ((370, 1224), 1, 5), ((374, 1238), 2, 1))

# the parent commit's own algorithm-to-algorithm difference for this very gradient -- the mean
# single-frame gradient of the three FRAMES under the default Winograd policy against MPSR_WINOGRAD_OFF, same weights
# (measured once, outside the suite: the policy is process-wide) -- and the same switch's difference of the total loss.
# At this width the switch makes no difference beyond what two runs under one policy differ by (7.4e-8 too), and the
# losses are equal to the last bit, so both bounds are their floors.  Measured for the batched step: 6.9e-6 and 2.4e-7.
YARDSTICK_GRAD = 7.4e-8
YARDSTICK_LOSS = 0.0
GRAD_BOUND = max(2e-5, 4 * YARDSTICK_GRAD)
LOSS_BOUND = max(1e-5, 4 * YARDSTICK_LOSS)


def _rel(a, b):  # (tests/test_sharded_training_step_gpu.py)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def frame(seed, n, size=(375, 1242), cam=0, full_trunk=True):
    from monopsr_amd.core import trainer
    rng = np.random.default_rng(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    H, Wd = size
    y1, x1 = rng.uniform(100, 200, n), rng.uniform(100, 900, n)
    boxes = np.stack([y1, x1, y1 + rng.uniform(40, 120, n), x1 + rng.uniform(60, 200, n)], 1).astype(np.float32)
    s = dict(boxes_2d=dev(boxes), cam_p=dev(CAMS[cam]),
             est_view_angs=dev(rng.uniform(-0.5, 0.5, n).astype(np.float32)),
             class_indices=torch.ones((n, 1), dtype=torch.int32, device="cuda"),
             mean_lwh=dev(np.tile(np.array([[3.88, 1.63, 1.53]], np.float32), (n, 1))),
             prop_cen_z_offset=torch.full((n,), 2.178, device="cuda"))
    if full_trunk:
        s["rgb_image"] = dev(rng.integers(0, 256, (H, Wd, 3)).astype(np.float32))
        s["boxes_2d_norm"] = dev(boxes / np.array([H, Wd, H, Wd], np.float32))
    else:
        s["rgb_image_crops"] = dev((rng.standard_normal((n, 48, 48, 3)) * 50).astype(np.float32))
        s["full_img_feature_crop"] = dev(np.maximum(rng.standard_normal((n, 12, 12, 1024 // DIV)), 0).astype(np.float32))
    s.update(trainer.synthetic_ground_truth(s, seed=seed + 1))
    return s


def three_frames():
    return [frame(50 + i, n, size, cam) for i, (size, cam, n) in enumerate(FRAMES)]


def make_trainer(decoder_bn, lr=0.0):
    from monopsr_amd.core import config_utils, train_net, trainer
    from monopsr_amd.core import weights as W
    cfg = config_utils.default_config()
    net = train_net.TrainNet(W.synthetic_weights(seed=43, width_div=DIV, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                             width_div=DIV, full_trunk=True, decoder_bn=decoder_bn)
    return trainer.InstanceTrainer(net, cfg.model_config, cfg.dataset_config, lr=lr)


@pytest.fixture(scope="module")
def trainers():
    made = {}

    def get(decoder_bn):
        if decoder_bn not in made:
            tr = make_trainer(decoder_bn)
            made[decoder_bn] = (tr, tr.net.params.clone())
        return made[decoder_bn][0]
    yield get
    for tr, params0 in made.values():  # lr = 0: no step moved a parameter
        assert torch.equal(tr.net.params, params0)


@pytest.fixture(scope="module")
def single_steps(trainers):
    """The three frames' own steps, computed once: (frames, [losses_dict as floats], [total], mean gradient)."""
    tr = trainers('frozen')
    frames = three_frames()
    dicts, totals, grads = [], [], []
    for s in frames:
        totals.append(float(tr.step(s)))
        dicts.append({k: float(v) for k, v in tr.losses_dict.items()})
        grads.append(tr.net.grads.clone())
    return frames, dicts, totals, (sum(grads) / len(grads)).cpu().numpy()


@pytest.mark.parametrize("decoder_bn", ["frozen", "batch"])
def test_one_frame_batch_is_the_single_step(trainers, decoder_bn):
    tr = trainers(decoder_bn)
    s = frame(50 + 1, 5, (370, 1224), 1)
    params0 = tr.net.params.clone()
    step0 = tr.global_step
    want_loss = float(tr.step(s))
    want = tr.net.grads.cpu().numpy().copy()
    got_loss = float(tr.step_batch([s]))
    got = tr.net.grads.cpu().numpy()
    assert tr.global_step == step0 + 2
    assert tr.model.frame_counts == [5] and tr.model.frame_index.dtype == torch.int32
    print("one frame, %s: loss %.3e, grads %.3e" % (decoder_bn, abs(got_loss - want_loss) / abs(want_loss),
                                                     _rel(got, want)))
    assert np.isfinite(want_loss) and np.abs(want).max() > 0
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    assert _rel(got, want) < 2e-5
    assert torch.equal(tr.net.params, params0)


def test_three_frame_gradient_is_the_mean_of_the_frames_gradients(trainers, single_steps):
    tr = trainers('frozen')
    frames, _, _, mean_grad = single_steps
    step0 = tr.global_step
    tr.step_batch(frames)
    assert tr.global_step == step0 + 1
    assert tr.model.frame_counts == [2, 5, 1]
    assert tr.model.frame_index.tolist() == [0, 0, 1, 1, 1, 1, 1, 2]
    err = _rel(tr.net.grads.cpu().numpy(), mean_grad)
    print("three frames: grads %.3e (bound %.3e)" % (err, GRAD_BOUND))
    assert np.abs(mean_grad).max() > 0
    assert err < GRAD_BOUND


def test_three_frame_losses_are_the_mean_of_the_frames_losses(trainers, single_steps):
    tr = trainers('frozen')
    frames, dicts, totals, _ = single_steps
    got_total = float(tr.step_batch(frames))
    got = {k: float(v) for k, v in tr.losses_dict.items()}
    assert set(got) == set(dicts[0]) and len(got) >= 8
    for k in got:
        want = float(np.mean([d[k] for d in dicts]))
        print("three frames: %s %.3e" % (k, abs(got[k] - want) / abs(want)))
        assert abs(got[k] - want) <= LOSS_BOUND * abs(want), (k, got[k], want)
    want = float(np.mean(totals))
    print("three frames: total %.3e (bound %.3e)" % (abs(got_total - want) / abs(want), LOSS_BOUND))
    assert abs(got_total - want) <= LOSS_BOUND * abs(want)


def test_batch_statistics_are_those_of_all_boxes(trainers):
    """decoder_bn='batch', crops route: two frames of 3 and 4 boxes that share a camera give the maps of ONE sample holding
    the seven boxes (same shapes, same kernels); the camera does not reach the decoder."""
    from monopsr_amd.core import constants
    tr = trainers('batch')
    key = constants.KEY_INST_XYZ_MAP_LOCAL
    a, b = frame(70, 3, cam=1, full_trunk=False), frame(71, 4, cam=1, full_trunk=False)
    pooled = {k: (a[k] if k == 'cam_p' else torch.cat([a[k], b[k]], 0)) for k in a}
    with torch.no_grad():
        want = tr.model.build(pooled)[0][key].cpu().numpy()
        got = tr.model.build_train_batch([a, b])[key].cpu().numpy()
        alone = tr.model.build(a)[0][key].cpu().numpy()
        b2 = dict(b, cam_p=torch.from_numpy(CAMS[2]).cuda())
        other = tr.model.build_train_batch([a, b2])
        cen_x = tr.model.build_train_batch([a, b])[constants.KEY_CEN_X]
    assert got.shape == (7, 48, 48, 3) and np.abs(want).max() > 0
    print("pooled statistics: maps %.3e" % _rel(got, want))
    assert _rel(got, want) < 2e-5
    assert _rel(got[:3], alone) > 1e-3  # frame A with its own statistics is something else
    assert np.array_equal(other[key].cpu().numpy(), got)  # same launches on the same inputs
    assert not torch.equal(other[constants.KEY_CEN_X][3:], cen_x[3:])  # (the heads do see it)


# ---------------------------------------------------------------------------------------------- from the dataset
# the five-frame split of tests/test_kitti_dataset_gpu.py's `root` fixture
SPLIT = (('000000', '000000'), ('000006', '000006'), ('000001', '000001'), ('000010', '000006'), ('000002', '000002'))
FILTER = dict(difficulty_str='all', box_2d_height=None, truncation=None, occlusion=None, depth_range=[5, 80])


@pytest.fixture(scope='module')
def root(tmp_path_factory):
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


def test_step_batch_on_a_dataset_batch(root):
    from monopsr_amd.core.config_utils import ConfigObj
    from monopsr_amd.datasets.kitti import kitti_dataset
    cfg = ConfigObj(dict(name='kitti', dataset_dir=root, data_split='train', data_split_dir='training', num_boxes=8,
                         classes=['Car'], oversample=True, num_alpha_bins=12, alpha_bin_overlap=0.0,
                         use_mscnn_detections=True, obj_filter_config=dict(FILTER),
                         aug_config=dict(use_image_aug=False, box_jitter_type='oversample'),
                         depth_version='multiscale', instance_version='depth_2_multiscale'))
    ds = kitti_dataset.KittiDataset(cfg, 'train', seed=0)
    tr = make_trainer('frozen', lr=1e-4)
    params0 = tr.net.params.clone()
    batch = ds.next_batch(3, True)
    assert len(batch) == 3
    loss = float(tr.step_batch(batch))
    assert np.isfinite(loss)
    assert tr.global_step == 1 and tr.model.frame_counts == [8, 8, 8]
    assert ds.status() == (0, 0)
    assert bool(torch.isfinite(tr.net.params).all()) and not torch.equal(tr.net.params, params0)
