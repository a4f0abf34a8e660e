"""The fused EMD loss returns the same bits on every call: its per-workgroup partial costs are added in workgroup order
(float32 atomics stood there before, and the evaluator's per-object EMD moved by one ulp from pass to pass).  That it is the cost of the materialised match is
tests/test_ops_gpu.py::test_emd_fused_loss_equals_the_three_ops."""
import pytest
import torch

from monopsr_amd.tf_ops.approxmatch import tf_approxmatch

pytestmark = pytest.mark.gpu


# 2304 points: nine / five workgroups per cloud (the evaluator's clouds); 300 x 700: ragged, two / one; 40: one
@pytest.mark.parametrize('semantics', ['device', 'host'])
@pytest.mark.parametrize('b,n,m', [(3, 2304, 2304), (2, 300, 700), (1, 40, 40)])
def test_cost_and_gradients_are_the_same_bits_on_every_call(b, n, m, semantics):
    g = torch.Generator(device='cuda').manual_seed(b * 1000 + n)
    x1 = torch.rand((b, n, 3), device='cuda', generator=g) * 2 - 1
    x2 = torch.rand((b, m, 3), device='cuda', generator=g) * 2 - 1
    first = [t.cpu().numpy().tobytes() for t in tf_approxmatch.emd_loss_fwd_bwd(x1, x2, semantics)]
    for _ in range(5):
        again = [t.cpu().numpy().tobytes() for t in tf_approxmatch.emd_loss_fwd_bwd(x1, x2, semantics)]
        assert again == first
    cost_only = tf_approxmatch.emd_loss_fwd_bwd(x1, x2, semantics, want_grads=False)[0]
    assert cost_only.cpu().numpy().tobytes() == first[0]
