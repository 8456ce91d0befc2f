"""CPU: the host side of the blended / flip-averaged stitch -- the float64 restatement the GPU tests compare against
(tests/stitch_restate.py) pinned to the reference's stitch (oracle/stitch_oracle.py) in the mode they share, the properties of the new
modes on that restatement, the two entry points' declaration / prototype / export, their argument checks (which launch nothing), and the
keyword validation of stitch_subvolumes, which runs before any device access."""
import os
import re

import numpy as np
import pytest
import torch

import stitch_restate as R
from oracle import stitch_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (12, 10, 9)
STRIDES = [(5, 4, 3), (7, 6, 1)]


def _vol(seed=11):
    return np.random.default_rng(seed).uniform(-1, 1, R.VOL + (1,))


@pytest.mark.parametrize('stride', STRIDES)
@pytest.mark.parametrize('process_img', [False, True])
def test_restatement_in_count_mode_is_the_reference_stitch(stride, process_img):
    vol = _vol()
    ref = S.stitch_subvolumes(R.probe_gen, vol.astype(np.float32), (1,) + K + (1,), stride=stride, complete=True, padFactor=0.25,
                              process_img=process_img)
    got = R.stitch(R.probe_gen, vol.astype(np.float32), K, stride=stride, complete=True, padFactor=0.25, process_img=process_img)
    assert got['out'].shape == ref.shape == R.VOL + (1,)
    assert not np.isnan(ref).any() and not np.isnan(got['out']).any()
    err = np.abs(got['out'] - ref).max()
    print('restatement vs stitch_oracle (0..255): %.2e' % err)
    assert err < 1e-3                     # the oracle accumulates in fp32; measured up to 6.0e-5


def test_window_walk_and_masks_agree_with_the_engine():
    from van_gan_amd.inference import flip_masks, gaussian_weights, window_origins
    for n, k, s in [(43, 12, 5), (33, 10, 4), (25, 9, 3), (17, 9, 1), (128, 128, 25), (306, 128, 50), (152, 128, 50)]:
        assert R.origins_1d(n, k, s) == window_origins(n, k, s)
    assert flip_masks(()) == flip_masks('') == [0] and flip_masks('x') == [0, 1] and flip_masks('zy') == flip_masks(['y', 'z']) == [0, 2, 4, 6]
    assert flip_masks('xyz') == list(range(8)) and flip_masks('xz') == [0, 1, 4, 5]
    for tta in ('', 'x', 'zy', 'xyz', 'xz'):
        assert R.flip_masks(tta) == flip_masks(tta)
    for k, sc in [(12, 0.125), (9, 0.125), (128, 0.25)]:
        w = gaussian_weights(k, sc)
        assert w.dtype == np.float32 and w.shape == (k,) and np.array_equal(w, w[::-1]) and np.array_equal(w.astype(np.float64), R.axis_weights(k, sc))
        i = k // 3
        assert w[i] == np.float32(np.exp(-0.5 * ((i - (k - 1) / 2) / (sc * k)) ** 2))
    # a narrow Gaussian is floored, not allowed to underflow to 0 (0/0 in the division); the product of three stays a normal fp32 number
    w = gaussian_weights(128, 0.01)
    assert w.min() == np.float32(1e-12) and w.max() > 0.9 and np.float32(w.min() * w.min()) * w.min() > np.finfo(np.float32).tiny
    assert np.array_equal(w.astype(np.float64), R.axis_weights(128, 0.01))
    narrow = R.stitch(R.probe_gen, _vol(), K, stride=(12, 10, 9), complete=False, blend='gaussian', sigma_scale=0.01)
    assert np.isfinite(narrow['out']).all()
    assert flip_masks(None) == [0]


def test_modes_on_the_restatement():
    vol = _vol()
    kw = dict(stride=STRIDES[0], complete=True, padFactor=0.25, process_img=True)
    base = R.stitch(R.probe_gen, vol, K, **kw)
    assert base['n_max'] == 36
    res = {}
    for blend, tta in [('gaussian', ''), ('count', 'x'), ('count', 'zy'), ('gaussian', 'xyz'), ('count', 'xyz')]:
        r = res[blend, tta] = R.stitch(R.probe_gen, vol, K, blend=blend, tta=tta, **kw)
        assert not np.isnan(r['out']).any()
        assert r['n_max'] == 36 * 2 ** len(tta) and r['forwards'] == base['forwards'] * 2 ** len(tta)
        d = np.abs(r['out'] - base['out']).max()
        print('%-8s tta=%-3r differs from count by %.1f on 0..255' % (blend, tta, d))
        assert d > 5.0                    # a mix-up between modes cannot pass a GPU comparison (bounds there are ~1e-2)
    modes = list(res)
    for a in range(len(modes)):
        for b in range(a + 1, len(modes)):
            assert np.abs(res[modes[a]]['out'] - res[modes[b]]['out']).max() > 1.0, (modes[a], modes[b])
    assert res['gaussian', 'xyz']['n_max'] == 288
    # a flip-equivariant generator: averaging over flips changes nothing
    for blend in ('count', 'gaussian'):
        e0 = R.stitch(R.equivariant_gen, vol, K, blend=blend, **kw)
        e8 = R.stitch(R.equivariant_gen, vol, K, blend=blend, tta='xyz', **kw)
        assert np.abs(e8['out'] - e0['out']).max() < 1e-9
    # a very wide Gaussian is the equal-weight stitch
    wide = R.stitch(R.probe_gen, vol, K, blend='gaussian', sigma_scale=1e4, **kw)
    assert np.abs(wide['out'] - base['out']).max() < 1e-9


def test_entry_points_declared_prototyped_and_exported():
    from van_gan_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'vangan_hip.h')).read()
    for name, nargs in (('vg_window_gather', 11), ('vg_window_scatter', 18)):
        assert re.search(r'^int\s+%s\s*\(' % name, hdr, flags=re.M), name
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert hasattr(_lib.lib, name) and hasattr(_lib.lib_fp16(), name)
    from van_gan_amd import build
    assert 'vg_stitch.hip' in build.SOURCES


def test_entry_checks_launch_nothing():
    from van_gan_amd._lib import lib, lib_fp16
    p = 1 << 20                           # never dereferenced: every call below is rejected on its arguments
    for L in (lib, lib_fp16()):
        g = lambda **o: L.vg_window_gather(*[o.get(n, d) for n, d in (('vol', p), ('X', 29), ('Y', 23), ('Z', 17), ('tab', p), ('B', 2), ('kx', 12),
                                                                     ('ky', 10), ('kz', 9), ('out', p), ('stream', None))])
        for bad in (dict(vol=None), dict(tab=None), dict(out=None), dict(B=0), dict(kx=0), dict(ky=0), dict(kz=-1), dict(kx=30), dict(ky=24), dict(kz=18)):
            assert g(**bad) == -1, bad
        s = lambda **o: L.vg_window_scatter(*[o.get(n, d) for n, d in (('win', p), ('tab', p), ('B', 2), ('kx', 12), ('ky', 10), ('kz', 9), ('px', 1),
                                                                      ('py', 1), ('pz', 0), ('wx', None), ('wy', None), ('wz', None), ('X', 29), ('Y', 23),
                                                                      ('Z', 17), ('pred', p), ('cnt', p), ('stream', None))])
        for bad in (dict(win=None), dict(tab=None), dict(pred=None), dict(cnt=None), dict(B=0), dict(kx=0), dict(kz=0), dict(kx=30), dict(ky=24),
                    dict(kz=18), dict(px=6), dict(py=5), dict(pz=5), dict(px=-1), dict(wx=p), dict(wx=p, wy=p), dict(wy=p, wz=p), dict(wz=p)):
            assert s(**bad) == -1, bad


def test_keyword_validation_needs_no_device():
    from van_gan_amd.inference import stitch_subvolumes
    img = torch.zeros(R.VOL + (1,))
    for kw in (dict(blend='linear'), dict(blend=None), dict(blend='gaussian', sigma_scale=0.0), dict(sigma_scale=-0.1),
               dict(sigma_scale=float('nan')), dict(sigma_scale=float('inf')), dict(sigma_scale='wide'), dict(tta='w'), dict(tta='xx'),
               dict(tta=('x', 'y', 'x')), dict(tta=['xy']), dict(tta=(0,)), dict(tta=3), dict(tta=1.5)):
        with pytest.raises(ValueError):
            stitch_subvolumes(None, 'gen_IS', img, K, **kw)         # engine None: any device access would be an AttributeError


def test_table_validation_on_the_host():
    from van_gan_amd.inference import _check_table
    for k in (K, (8, 8, 16)):
        assert np.array_equal(_check_table(R.table(k), R.VOL, k), R.table(k))
        assert np.array_equal(_check_table(torch.from_numpy(R.table(k)), R.VOL, k), R.table(k))
    good = R.table(K)
    for row, col, val in [(0, 0, -1), (3, 0, 18), (2, 1, 14), (5, 2, 9), (1, 3, 8), (1, 3, -1)]:
        t = good.copy()
        t[row, col] = val
        with pytest.raises(ValueError):
            _check_table(t, R.VOL, K)
    for bad in (good[:, :3], good[:0], good.astype(np.float32)):
        with pytest.raises(ValueError):
            _check_table(bad, R.VOL, K)
    with pytest.raises(ValueError):
        _check_table(good, R.VOL, (30, 10, 9))
