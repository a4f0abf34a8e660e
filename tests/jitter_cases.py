"""The seeded boxes on which the jitter kernel is compared with its restatement (tests/test_kitti_aug_gpu.py); the CPU
suite checks that no trial of the restatement lands within 1e-9 of the threshold on them (tests/test_kitti_aug.py)."""
import numpy as np

SIZES = ((375, 1242), (370, 1224), (374, 1238))
THRESHOLDS = (0.5, 0.7, 0.9)
P2 = {(375, 1242): (721.5377, 609.5593), (370, 1224): (707.0493, 604.0814), (374, 1238): (718.3351, 600.3891)}
PER_CASE = 2400


def _case(k, hw, thr, seed, epoch):
    h, w = hw
    rng = np.random.default_rng(1000 + k)
    n = PER_CASE
    bw, bh = rng.uniform(2, 600, n), rng.uniform(2, 370, n)
    x1, y1 = rng.uniform(0, w - 1 - np.minimum(bw, w - 1)), rng.uniform(0, h - 1 - np.minimum(bh, h - 1))
    b = np.stack([x1, y1, np.minimum(x1 + bw, w - 1), np.minimum(y1 + bh, h - 1)], 1)
    b[0::11, 0] = 0.0        # boxes touching every border of the image
    b[1::11, 1] = 0.0
    b[2::11, 2] = w - 1
    b[3::11, 3] = h - 1
    b[4::44] = [0.0, 0.0, w - 1, h - 1]
    b = b.astype(np.float32).astype(np.float64)  # label files hold float32 values
    flags = (np.arange(n) % 6 != 5).astype(np.int32)
    return dict(boxes=b, flags=flags, hw=np.tile(np.array(hw, np.int32), (n, 1)),
                p=np.tile(np.array(P2[hw]), (n, 1)), frame_index=rng.integers(0, 7481, n).astype(np.int32),
                slot=(np.arange(n) % 32).astype(np.int32), seed=seed, epoch=epoch, thr=thr)


def cases():
    """Nine cases of 2400 boxes: three image sizes x three thresholds, with several epochs and seeds."""
    out = []
    for k, (hw, thr) in enumerate((hw, thr) for hw in SIZES for thr in THRESHOLDS):
        seed = (0, 1, 0xDEADBEEF12345678)[k % 3]
        out.append(_case(k, hw, thr, seed, epoch=(0, 1, 5, 37)[k % 4]))
    return out
