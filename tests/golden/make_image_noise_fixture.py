"""Records tests/golden/image_noise.npz: the outputs of the reference's own kitti_aug.apply_image_noise under
np.random.seed(s) on one 6 x 8 x 3 image that contains 0 and 255.  Needs the reference tree:
python make_image_noise_fixture.py <reference>/src.

The seeds are searched (on the CPU, by tests/image_noise_restatement.numpy_stream_draws, which consumes np.random as the
function does) so that every kind of call occurs: untouched, swap only, each noise stage as the last one, a swap that a
noise stage overwrites, and two or more noise stages firing.  The fixture holds the image, the seeds and the
function's outputs only."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_noise_restatement as nr  # noqa: E402

SHAPE = (6, 8, 3)


def _import_reference(src):
    sys.path.insert(0, src)
    # modules the reference imports at load time and apply_image_noise never calls: an empty stand-in for each missing
    # one
    for _ in range(64):
        try:
            from monopsr.datasets.kitti import kitti_aug
            return kitti_aug
        except ModuleNotFoundError as e:
            if e.name.split('.')[0] == 'monopsr':
                raise
            mod = types.ModuleType(e.name)
            mod.__path__ = []
            sys.modules[e.name] = mod
            if '.' in e.name:
                parent, _, leaf = e.name.rpartition('.')
                setattr(sys.modules[parent], leaf, mod)
            for key in [k for k in sys.modules if k.startswith('monopsr')]:
                del sys.modules[key]
    from monopsr.datasets.kitti import kitti_aug
    return kitti_aug


def image():
    img = np.random.default_rng(2024).integers(0, 256, SHAPE).astype(np.uint8)
    img[0, 0] = (0, 255, 0)
    img[5, 7] = (255, 0, 255)
    img[2, 3] = (3, 250, 128)
    return img


def kinds(fired):
    """The kinds of call a stage bitmask belongs to."""
    noise = [s for s in (nr.GAUSSIAN, nr.CHANNEL, nr.BRIGHTNESS, nr.UNIFORM) if fired >> s & 1]
    out = {'last_' + nr.outcome(fired)}
    if fired & 1 and noise:
        out.add('swap_overwritten')
    if len(noise) >= 2:
        out.add('two_or_more_noise_stages')
    return out


WANTED = ('last_untouched', 'last_swap', 'last_gaussian', 'last_channel', 'last_brightness', 'last_uniform',
          'swap_overwritten', 'two_or_more_noise_stages')


def search_seeds(per_kind=2, limit=100000):
    """The first seeds, in order, that bring every kind of WANTED up to per_kind occurrences."""
    count = {k: 0 for k in WANTED}
    seeds = []
    for s in range(limit):
        np.random.seed(s)
        found = kinds(nr.numpy_stream_draws(SHAPE)['fired'])
        if any(count[k] < per_kind for k in found):
            seeds.append(s)
            for k in found:
                count[k] += 1
        if all(c >= per_kind for c in count.values()):
            return seeds
    raise RuntimeError('seeds 0..%d leave %s short' % (limit, [k for k, c in count.items() if c < per_kind]))


def main(src):
    kitti_aug = _import_reference(src)
    img = image()
    seeds = search_seeds()
    outputs = []
    for s in seeds:
        np.random.seed(s)
        given = img.copy()
        outputs.append(np.array(kitti_aug.apply_image_noise(given), np.uint8))
        assert np.array_equal(given, img)
    np.savez_compressed(os.path.join(HERE, 'image_noise.npz'), image=img, seeds=np.asarray(seeds, np.int64),
                        outputs=np.stack(outputs))
    print('recorded %d seeds: %s' % (len(seeds), seeds))


if __name__ == '__main__':
    main(sys.argv[1])
