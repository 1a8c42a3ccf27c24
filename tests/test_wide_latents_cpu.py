"""The latent limit of the decomposed-KL kernels (64, the grid search's max_latents) is enforced by
the Python glue before anything reaches the library: no GPU needed."""

import pytest
import torch

from behavenet_amd import _hip
from behavenet_amd import hip_functions as hf


def _no_library():
    raise AssertionError('the library was reached')


@pytest.mark.parametrize('D', [65, 128])
def test_decomposed_kl_refuses_more_than_64_latents(monkeypatch, D):
    monkeypatch.setattr(_hip, 'load', _no_library)
    z, mu, lv = (torch.zeros((10, D), requires_grad=True) for _ in range(3))
    with pytest.raises(ValueError, match='at most 64'):
        hf.decomposed_kl_terms(z, mu, lv)
    with pytest.raises(ValueError, match='at most 64'):
        hf.decomposed_kl_chunks(z, mu, lv, [(0, 6), (6, 10)])
    with pytest.raises(ValueError, match='at most 64'):
        _hip.decomposed_kl_fwd(z.detach(), mu.detach(), lv.detach())
    with pytest.raises(ValueError, match='at most 64'):
        _hip.decomposed_kl_bwd(z.detach(), mu.detach(), lv.detach(), torch.zeros(10),
                               torch.zeros((10, D)), torch.ones(3))


def test_decomposed_kl_serves_up_to_64_latents(monkeypatch):
    """D = 64 passes the check and goes on to the library."""
    monkeypatch.setattr(_hip, 'load', _no_library)
    z = torch.zeros((10, 64))
    with pytest.raises(AssertionError, match='library was reached'):
        _hip.decomposed_kl_fwd(z, z, z)
