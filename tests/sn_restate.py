"""Float64 restatement of the spectrally normalised discriminator (get_discriminator(use_SN=True), discriminator.py:16,54-61,86,100;
building_blocks.py:172-180) for the tests: the oracle has no such discriminator.  TP (TensorFlow Addons' SpectralNormalization with
power_iterations = 1, restated from its definition -- TensorFlow Addons is not available to check against):

    l2n(x) = x * rsqrt(max(sum(x * x), 1e-12));  v = l2n(u W^T);  u' = l2n(v W);  sigma = (v W) u'^T;  u <- u';  W <- W / sigma

with W the Keras kernel [kd][kh][kw][Cin][Cout] viewed as [K, Cout] and u [1, Cout].  No gradient flows through u', v or sigma: the
variable is overwritten, the network below is the plain convolution stack on the projected kernels."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vangan_oracle as O

WRAPPED = ('conv0', 'down0', 'down1', 'down2')
SHAPES = ((64, 64), (4096, 128), (8192, 256), (16384, 512))        # [K = k^3 Cin, Cout] of the four wrapped kernels


def l2n(x):
    return x / np.sqrt(max(float((x * x).sum()), 1e-12))


def project(W, u, dtype=np.float64):
    """One projection: (W / sigma, u', sigma); W [K, Cout], u [1, Cout].  sigma == 0 leaves W and u as they are."""
    W, u = np.asarray(W, dtype=dtype), np.asarray(u, dtype=dtype)
    v = l2n(u @ W.T)
    s = v @ W
    u1 = l2n(s)
    sigma = float((s @ u1.T).item())
    if not sigma > 0.0:
        return W, u, 0.0
    return (W / dtype(sigma)).astype(dtype), u1.astype(dtype), sigma


def project_params(p, n=2):
    """n projections of the four wrapped kernels of one discriminator's parameter dict (torch tensors) -> new dict in float64, sigmas."""
    out = {k: v.double().clone() for k, v in p.items()}
    sig = {}
    for k in WRAPPED:
        W = out[k + '.w'].numpy().reshape(-1, out[k + '.w'].shape[-1])
        u = out[k + '.sn_u'].numpy()
        sig[k] = []
        for _ in range(n):
            W, u, s = project(W, u)
            sig[k].append(s)
        out[k + '.w'] = torch.from_numpy(np.ascontiguousarray(W)).reshape(out[k + '.w'].shape)
        out[k + '.sn_u'] = torch.from_numpy(np.ascontiguousarray(u))
    return out, sig


def he_normal(K, C, seed):
    """he_normal of a [K, C] kernel view (fan_in = K), truncated at 2 sigma, and a TruncatedNormal(0.02) u."""
    g = torch.Generator().manual_seed(seed)
    W = torch.empty(K, C); u = torch.empty(1, C)
    torch.nn.init.trunc_normal_(W, 0.0, 1.0, -2.0, 2.0, generator=g)
    torch.nn.init.trunc_normal_(u, 0.0, 1.0, -2.0, 2.0, generator=g)
    return W * ((2.0 / K) ** 0.5 / 0.87962566103423978), u * 0.02


def disc_forward(p, x_ndhwc, noise=None, drop=None, q=None):
    """reflect-pad -> noise -> Conv(64,k4,s2,bias) -> LReLU; down0 / down1 (k4 s2 behind reflect-pad + noise), down2 (k4 s1 'same'):
    Conv(no bias) -> LReLU -> SpatialDropout3D; noise -> Conv(1,k3,'same',bias) [-> Flatten -> Dropout -> Dense(1)].  The kernels
    are used as given (project them first).  q: O.bf16_round at the stored tensors (the bf16 engine) or None."""
    noise, drop = noise or {}, drop or {}

    def nz(k, t):
        return t + O.to_ncdhw(noise[k]) if noise.get(k) is not None else t

    x = O.to_ncdhw(x_ndhwc)
    h = O._store(q, 'conv0', O.conv3d(nz('conv0', O.reflect_pad1(x)), p['conv0.w'], p['conv0.b'], 2, 'valid', q))
    h = F.leaky_relu(h, O.LRELU_SLOPE)
    for i in range(3):
        k = 'down%d' % i
        if i < 2:
            h = O._store(q, k, O.conv3d(nz(k, O.reflect_pad1(h)), p[k + '.w'], None, 2, 'valid', q))
        else:
            h = O._store(q, k, O.conv3d(nz(k, h), p[k + '.w'], None, 1, 'same', q))
        h = F.leaky_relu(h, O.LRELU_SLOPE)
        if drop.get(k) is not None:
            h = h * drop[k].view(h.shape[0], h.shape[1], 1, 1, 1)
    y = O.conv3d(nz('out', h), p['out.w'], p['out.b'], 1, 'same', q)
    if 'dense.w' in p:
        f = O.to_ndhwc(y).reshape(y.shape[0], -1)
        if drop.get('head') is not None:
            f = f * drop['head']
        return f @ p['dense.w'] + p['dense.b']
    return O.to_ndhwc(y)


def disc_losses(d_real, d_fake, gbs, wasserstein=False):
    """(critic loss, generator loss) as oracle.compute_losses states them (vangan.py:322-332)."""
    if wasserstein:
        return -O.reduce_mean(d_real - d_fake, gbs), -O.reduce_mean(d_fake, gbs)
    d = 0.5 * (O.mse(torch.ones_like(d_real), d_real, gbs) + O.mse(torch.zeros_like(d_fake), d_fake, gbs))
    return d, O.mse(torch.ones_like(d_fake), d_fake, gbs)
