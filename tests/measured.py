"""``tests.test_gpu_kernels.close`` with its two figures printed first (pytest -s shows them): shared by the device
tests that record, per output, how much room the tolerance leaves (tests/test_gpu_linear.py,
tests/test_gpu_psvae_head.py)."""
import numpy as np

from tests.test_gpu_kernels import close


def measured_close(got, want, want64, name, sum_of=None):
    """``close`` unchanged, after printing e_hip and e_cpu: the largest error against float64 over the result's
    maximum, of the device result and of the fp32 CPU result."""
    w64 = want64.detach().cpu().double().numpy()
    scale = max(np.abs(w64).max(), 1e-30)
    e_hip = np.abs(got.detach().cpu().double().numpy() - w64).max() / scale
    e_cpu = np.abs(want.detach().cpu().double().numpy() - w64).max() / scale
    print('FIGURE %s: e_hip %.3e e_cpu %.3e' % (name, e_hip, e_cpu))
    close(got, want, want64, name=name, sum_of=sum_of)
