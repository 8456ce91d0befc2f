"""What the GPU suites of the preprocessing and the stitch share: the device, an upload, the raw stack of the end-to-end cases, the
recorder that stands in for the library handle, and the small engine.  Not a test module."""
import numpy as np
import torch

DEV = 'cuda:0'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raw(dtype, shape=(24, 20, 35)):
    rng = np.random.default_rng(len(dtype) + sum(shape))
    top = 255 if dtype == 'uint8' else 65535
    v = rng.gamma(2.0, 0.08, shape) * (1.0 + 0.3 * np.cos(np.arange(shape[2]) / 5.0))
    v += (rng.random(shape) < 0.02) * rng.random(shape)
    return np.clip(v * top, 0, top).astype(dtype)


class _Recorder:
    """Stands in for the library handle inside a module of van_gan_amd (preprocess, inference) and notes which entries are called."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def _engine():
    from van_gan_amd import VanGan
    return VanGan((32, 32, 32), batch_size=4, device=DEV, seed=5, precision='fp32')
