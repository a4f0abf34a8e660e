"""Image noise on the host: the restatement's arithmetic against a recording of the reference's own apply_image_noise,
the statistics of the counter-based draws, what the two modes share, and the options KittiDataset refuses.  No GPU."""
import os

import numpy as np
import pytest

import image_noise_restatement as nr
from monopsr_amd import _lib
from monopsr_amd.core.config_utils import ConfigObj
from monopsr_amd.datasets.kitti import kitti_aug, kitti_dataset

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, 'golden', 'image_noise.npz'))
SEED = 20240607


def _apply(image, d, mode):
    return nr.apply_stages(image, d['fired'], d['gaussian'], d['channel'], d['brightness'], d['uniform_noise'], mode)


def test_reference_mode_equals_the_recorded_reference_outputs():
    """Last stage wins, G := B and the truncation, against the function itself: the restatement fed with np.random's
    draws in the function's order gives the recorded bytes."""
    image, seeds, outputs = FIX['image'], FIX['seeds'], FIX['outputs']
    assert image.shape == (6, 8, 3) and image.dtype == np.uint8 and image.min() == 0 and image.max() == 255
    assert outputs.shape == (len(seeds), 6, 8, 3) and outputs.dtype == np.uint8
    seen = set()
    state = np.random.get_state()
    try:
        for s, want in zip(seeds, outputs):
            np.random.seed(int(s))
            d = nr.numpy_stream_draws(image.shape)
            got = _apply(image, d, 'reference')
            assert got.tobytes() == want.tobytes(), (int(s), d['fired'])
            fired = d['fired']
            noise = bin(fired >> 1).count('1')
            seen.add(nr.outcome(fired))
            if fired & 1 and noise:
                seen.add('swap overwritten')
            if noise >= 2:
                seen.add('two or more')
            if fired == 1:  # the "swap": G := B, and B stays
                assert np.array_equal(want[:, :, 1], image[:, :, 2]) and np.array_equal(want[:, :, 2], image[:, :, 2])
                assert np.array_equal(want[:, :, 0], image[:, :, 0])
            if fired == 0:
                assert np.array_equal(want, image)
    finally:
        np.random.set_state(state)
    assert seen == set(nr.OUTCOMES) | {'swap overwritten', 'two or more'}


def test_outcome_frequencies_of_the_counter_based_draws():
    n_epochs, n_frames = 100, 200
    total = n_epochs * n_frames
    assert total == 20000
    fired = nr.fired_of(SEED, np.arange(n_epochs)[:, None], np.arange(n_frames)[None, :]).reshape(-1)
    names = np.array([nr.outcome(int(f)) for f in fired])
    assert abs(sum(nr.OUTCOMES.values()) - 1.0) < 1e-12
    for name, p in nr.OUTCOMES.items():
        count = int((names == name).sum())
        se = np.sqrt(total * p * (1 - p))
        print('%-10s %5d of %d, expected %.1f +- %.1f' % (name, count, total, total * p, se))
        assert abs(count - total * p) <= 4 * se, (name, count, total * p, se)
    # fired_of is frame_draws, vectorised
    for e, f in ((0, 0), (3, 17), (99, 199)):
        assert nr.frame_draws(SEED, e, f)[0] == fired[e * n_frames + f]


def _first_coordinate(pred, epoch=0, limit=4000):
    fired = nr.fired_of(SEED, epoch, np.arange(limit))
    return next(int(f) for f in range(limit) if pred(int(fired[f])))


def test_gaussian_stage_on_mid_grey_has_the_moments_of_truncated_noise():
    """out - 128 = floor(10 z) for |10 z| < 128: mean -1/2, variance 100 + 1/12 (a rounding error uniform on [0, 1)
    and, to the precision that matters here, independent of z)."""
    frame = _first_coordinate(lambda f: nr.outcome(f) == 'gaussian')
    image = np.full((48, 64, 3), 128, np.uint8)
    out, fired, _ = nr.restate(image, SEED, 0, frame, 'reference')
    assert nr.outcome(fired) == 'gaussian'
    d = out.astype(np.float64) - 128.0
    n = d.size
    var = 100.0 + 1.0 / 12.0
    se_mean = np.sqrt(var / n)
    se_var = var * np.sqrt(2.0 / (n - 1))  # of a normal sample's variance
    print('mean %.4f (se %.4f), variance %.3f (se %.3f), n %d' % (d.mean(), se_mean, d.var(ddof=1), se_var, n))
    assert 0 < out.min() and out.max() < 255
    assert abs(d.mean() + 0.5) <= 4 * se_mean
    assert abs(d.var(ddof=1) - var) <= 4 * se_var


def test_composed_equals_reference_for_a_single_noise_stage_without_swap():
    rng = np.random.default_rng(5)
    image = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    image[0, 0], image[4, 6] = 0, 255
    fired = nr.fired_of(SEED, 2, np.arange(400))
    seen = set()
    for frame, f in enumerate(fired):
        a, _, _ = nr.restate(image, SEED, 2, frame, 'reference')
        b, _, _ = nr.restate(image, SEED, 2, frame, 'composed')
        if f in (2, 4, 8, 16):
            assert np.array_equal(a, b), (frame, f)
            seen.add(int(f))
        elif f == 0:
            assert np.array_equal(a, image) and np.array_equal(b, image)
    assert seen == {2, 4, 8, 16}
    # and they differ where the description and the function part ways: a swap, or two noise stages
    frame = _first_coordinate(lambda f: f == 1, epoch=2)
    a, _, _ = nr.restate(image, SEED, 2, frame, 'reference')
    b, _, _ = nr.restate(image, SEED, 2, frame, 'composed')
    assert np.array_equal(a[:, :, 2], image[:, :, 2]) and np.array_equal(b[:, :, 2], image[:, :, 1])
    assert np.array_equal(a[:, :, 1], image[:, :, 2]) and np.array_equal(b[:, :, 1], image[:, :, 2])
    frame = _first_coordinate(lambda f: f & 1 == 0 and bin(f).count('1') >= 2, epoch=2)
    assert not np.array_equal(nr.restate(image, SEED, 2, frame, 'reference')[0],
                              nr.restate(image, SEED, 2, frame, 'composed')[0])


def test_composed_swap_twice_is_the_identity():
    image = np.random.default_rng(6).integers(0, 256, (4, 5, 3)).astype(np.uint8)
    once = nr.apply_stages(image, 1, None, None, None, None, 'composed')
    assert not np.array_equal(once, image)
    assert np.array_equal(once[:, :, 1], image[:, :, 2]) and np.array_equal(once[:, :, 2], image[:, :, 1])
    assert np.array_equal(nr.apply_stages(once, 1, None, None, None, None, 'composed'), image)
    # the reference's "swap" is not an involution
    twice = nr.apply_stages(nr.apply_stages(image, 1, None, None, None, None, 'reference'), 1, None, None, None, None,
                            'reference')
    assert not np.array_equal(twice, image)


def test_philox_draws_pair_layout():
    """Elements 2q, 2q + 1 come from counter c0 = q whatever the shape, so a frame's noise does not depend on how its
    elements are grouped; an odd frame's last pair is half a pair."""
    a = nr.philox_draws(SEED, 1, 9, (5, 7, 3))
    b = nr.philox_draws(SEED, 1, 9, (35, 1, 3))
    c = nr.philox_draws(SEED, 1, 9, (6, 6, 3))
    for k in ('gaussian', 'uniform_noise'):
        assert np.array_equal(a[k].reshape(-1), b[k].reshape(-1))
        assert np.array_equal(a[k].reshape(-1), c[k].reshape(-1)[:105])
    assert a['fired'] == c['fired'] and np.array_equal(a['params'], c['params'])
    assert 0 <= a['params'][0] < 10 and (np.abs(a['uniform_noise']) <= a['params'][0]).all()


# ---- the options


def _config(tmp_path, **aug):
    (tmp_path / 'training').mkdir(exist_ok=True)
    (tmp_path / 'train.txt').write_text('000000\n')
    return ConfigObj(dict(
        dataset_dir=str(tmp_path), data_split='train', data_split_dir='training', num_boxes=8, classes=['Car'],
        oversample=True, num_alpha_bins=12, alpha_bin_overlap=0.0, use_mscnn_detections=False,
        obj_filter_config=dict(kitti_dataset.DEFAULT_OBJ_FILTER),
        aug_config=dict(dict(use_image_aug=True, box_jitter_type='oversample'), **aug), depth_version='multiscale',
        instance_version='depth_2_multiscale'))


def test_image_noise_option_errors(tmp_path):
    # use_image_aug without a choice: the error names the switch and both choices
    with pytest.raises(ValueError) as e:
        kitti_dataset.KittiDataset(_config(tmp_path), 'train')
    assert 'use_image_aug' in str(e.value) and "'reference'" in str(e.value) and "'composed'" in str(e.value)
    # an unknown value, from the config or from the argument, names image_noise
    with pytest.raises(ValueError, match='image_noise'):
        kitti_dataset.KittiDataset(_config(tmp_path, image_noise='sideways'), 'train')
    with pytest.raises(ValueError, match='image_noise'):
        kitti_dataset.KittiDataset(_config(tmp_path), 'train', image_noise='both')
    with pytest.raises(ValueError, match='image_noise'):
        kitti_aug.image_noise_mode(None)
    assert kitti_aug.image_noise_mode('reference') == 1 and kitti_aug.image_noise_mode('composed') == 2
    assert kitti_aug.IMAGE_NOISE_STAGES == ('swap', 'gaussian', 'channel', 'brightness', 'uniform')


def test_image_noise_options_that_pass_the_check():
    ds = kitti_dataset.KittiDataset.__new__(kitti_dataset.KittiDataset)
    ds.box_jitter_type, ds.use_mscnn_detections, ds.oversample, ds.num_classes = None, False, True, 1
    for mode, aug, choice, want in (('train', True, 'reference', 1), ('train', True, 'composed', 2),
                                    ('train', False, 'composed', 0), ('val', True, 'reference', 0),
                                    ('val', True, None, 0)):
        ds.train_val_test, ds.use_image_aug, ds.image_noise = mode, aug, choice
        ds._check_options()
        assert ds.image_noise_mode == want
    # a bare instance without the attribute, as long as use_image_aug is off
    del ds.image_noise
    ds.train_val_test, ds.use_image_aug = 'train', False
    ds._check_options()
    assert ds.image_noise_mode == 0


def test_apply_image_noise_refuses_float_input_and_unknown_modes():
    with pytest.raises(_lib.InvalidArgumentError, match='uint8'):
        kitti_aug.apply_image_noise(np.zeros((4, 4, 3), np.float32), 0)
    with pytest.raises(ValueError, match='image_noise'):
        kitti_aug.apply_image_noise(np.zeros((4, 4, 3), np.uint8), 0, mode='meant')
    with pytest.raises(_lib.InvalidArgumentError, match='h, w, 3'):
        kitti_aug.apply_image_noise(np.zeros((4, 4), np.uint8), 0)


def test_abi_12_declares_the_entry_point():
    assert _lib.ABI_VERSION == 13 and 'mpsr_image_noise' in _lib.SIGNATURES
