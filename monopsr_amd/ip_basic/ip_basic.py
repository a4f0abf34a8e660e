"""IP-Basic's multi-scale depth completion (src/ip_basic/ip_basic.py:40-193) on the GPU, on the reference's names.

    depths, process_dict = fill_in_multiscale(projected_depths)            # (H, W) numpy -> numpy, or CUDA tensor
    depths, stages = fill_in_multiscale_batch(maps, show_process=True)     # (F, H, W) CUDA tensor or numpy

The whole chain (binned dilations, closing, medians, hole fills, the six masked dilations, the bilateral or gaussian
blur and the inversions) runs as HIP kernels (mpsr_depth_fill_multiscale); there is no CPU path, and CPU tensors are
refused.  Results equal the reference run on cv2 with the semantics DESIGN.md section 7.2 lists; the stages s1 .. s8 of
show_process come from the same launch chain.
"""
import collections
import ctypes

import numpy as np

from monopsr_amd import _lib

FULL_KERNEL_5 = np.ones((5, 5), np.uint8)
FULL_KERNEL_7 = np.ones((7, 7), np.uint8)
FULL_KERNEL_9 = np.ones((9, 9), np.uint8)
FULL_KERNEL_31 = np.ones((31, 31), np.uint8)
CROSS_KERNEL_3 = np.asarray([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=np.uint8)
CROSS_KERNEL_5 = np.asarray([[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]],
                            dtype=np.uint8)
CROSS_KERNEL_7 = np.zeros((7, 7), np.uint8)
CROSS_KERNEL_7[3, :] = 1
CROSS_KERNEL_7[:, 3] = 1

MAX_KERNEL = 15  # MPSR_DEPTH_MAX_KERNEL
BLUR_TYPES = {'bilateral': 0, 'gaussian': 1}  # MPSR_DEPTH_BLUR_*
STAGE_NAMES = ('s1_inverted_depths', 's2_dilated_depths', 's3_closed_depths', 's4_blurred_depths',
               's5_combined_depths', 's6_extended_depths', 's7_blurred_depths', 's8_inverted_depths')


def _opts(max_depth, kernels, extrapolate, blur_type):
    if blur_type not in BLUR_TYPES:
        raise _lib.InvalidArgumentError('blur_type must be one of %s, got %r' % (sorted(BLUR_TYPES), blur_type))
    o = _lib.DepthFillOpts()
    o.max_depth = float(max_depth)
    o.extrapolate = int(bool(extrapolate))
    o.blur_type = BLUR_TYPES[blur_type]
    for b, k in enumerate(kernels):
        k = np.asarray(k)
        if k.ndim != 2:
            raise _lib.InvalidArgumentError('dilation kernels are 2-D, got shape %s' % (k.shape,))
        kh, kw = k.shape
        o.kernel_h[b], o.kernel_w[b] = kh, kw  # sizes outside 1..15 are refused by the library
        if 1 <= kh <= MAX_KERNEL and 1 <= kw <= MAX_KERNEL:
            for i in range(kh):
                for j in range(kw):
                    o.kernels[b][i * MAX_KERNEL + j] = 1 if k[i, j] else 0
    return o


def fill_in_multiscale_batch(depth_maps, max_depth=100.0, dilation_kernel_far=CROSS_KERNEL_3,
                             dilation_kernel_med=CROSS_KERNEL_5, dilation_kernel_near=CROSS_KERNEL_7,
                             extrapolate=False, blur_type='bilateral', show_process=False):
    """fill_in_multiscale of F frames of one size in one launch chain: (F, H, W) -> (depths (F, H, W), stages or None).

    depth_maps: a CUDA tensor (any float dtype; converted to float32) or a numpy array, which is uploaded to the
    current device and answered in numpy.  stages: (F, 8, H, W) = s1 .. s8 when show_process, else None."""
    import torch
    as_numpy = isinstance(depth_maps, np.ndarray)
    if as_numpy:
        t = torch.from_numpy(np.ascontiguousarray(depth_maps, np.float32)).cuda()
    elif torch.is_tensor(depth_maps):
        if not depth_maps.is_cuda:
            raise _lib.InvalidArgumentError('fill_in_multiscale: expected a CUDA tensor or a numpy array, got a CPU '
                                            'tensor (monopsr_amd has no CPU path)')
        t = depth_maps.to(torch.float32).contiguous()
    else:
        raise _lib.InvalidArgumentError('fill_in_multiscale: expected a CUDA tensor or a numpy array')
    if t.dim() != 3:
        raise _lib.InvalidArgumentError('fill_in_multiscale_batch: expected (F, H, W), got %s' % (tuple(t.shape),))
    nf, h, w = t.shape
    opts = _opts(max_depth, (dilation_kernel_far, dilation_kernel_med, dilation_kernel_near), extrapolate, blur_type)
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        out = torch.empty_like(t)
        stages = torch.empty((nf, 8, h, w), dtype=torch.float32, device=t.device) if show_process else None
        ws = torch.empty(max(1, lib.mpsr_depth_fill_workspace_bytes(nf, h, w)), dtype=torch.uint8, device=t.device)
        _lib.check(lib.mpsr_depth_fill_multiscale(_lib.ptr(t), nf, h, w, ctypes.byref(opts), _lib.ptr(out),
                                                  _lib.ptr(stages), _lib.ptr(ws), ws.numel(), _lib.stream()))
    if as_numpy:
        return out.cpu().numpy(), (stages.cpu().numpy() if stages is not None else None)
    return out, stages


def fill_in_multiscale(depth_map, max_depth=100.0, dilation_kernel_far=CROSS_KERNEL_3,
                       dilation_kernel_med=CROSS_KERNEL_5, dilation_kernel_near=CROSS_KERNEL_7, extrapolate=False,
                       blur_type='bilateral', show_process=False):
    """The reference's fill_in_multiscale: (H, W) projected depths -> (dense depths, process_dict or None).

    numpy in, numpy out; a CUDA tensor in, tensors out.  process_dict (show_process) holds s0_depths_in, s1 .. s8 and
    s9_depths_out under the reference's keys."""
    import torch
    if isinstance(depth_map, np.ndarray):
        batch = np.asarray(depth_map, np.float32)[None]
    elif torch.is_tensor(depth_map):
        batch = depth_map[None]
    else:
        raise _lib.InvalidArgumentError('fill_in_multiscale: expected a CUDA tensor or a numpy array')
    if batch.ndim != 3:
        raise _lib.InvalidArgumentError('fill_in_multiscale: expected (H, W), got %s' % (tuple(depth_map.shape),))
    out, stages = fill_in_multiscale_batch(batch, max_depth, dilation_kernel_far, dilation_kernel_med,
                                           dilation_kernel_near, extrapolate, blur_type, show_process)
    process_dict = None
    if show_process:
        process_dict = collections.OrderedDict()
        process_dict['s0_depths_in'] = batch[0]
        for k, name in enumerate(STAGE_NAMES):
            process_dict[name] = stages[0, k]
        process_dict['s9_depths_out'] = out[0]
    return out[0], process_dict
