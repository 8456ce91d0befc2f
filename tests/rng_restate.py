"""Restatement of the device RNG in numpy -- test infrastructure only, not a test module.

Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11, section 4 and the Random123
definition): a 128-bit counter (c0, c1, c2, c3) and a 64-bit key (k0, k1).  One round is

    (hi0, lo0) = 0xD2511F53 * c0        (hi1, lo1) = 0xCD9E8D57 * c2          (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)

and between two rounds the key advances by the Weyl constants (0x9E3779B9, 0xBB67AE85): ten rounds, nine key bumps.

The streams of include/vangan_hip.h (vg_randn_bf16, vg_dropout_mask):

    counter = (lo32(offset + i), hi32(offset + i), domain, 0), key = (lo32(seed), hi32(seed));  offset + i wraps at 2^64
    domain  = 0x5eed for the Gaussian noise, 0xd60b for the dropout masks
    u01(x)  = ((x >> 8) + 0.5) * 2^-24 in float32: 24 bits, never 0 (so the logarithm is finite); 2^24 - 0.5 is no float32 and rounds to
              even, i.e. the largest value is exactly 1.0
    mask    : element i is dropped where u01(word 0 of counter i) < rate, kept elements are 1 / (1 - rate)
    noise   : counter q gives four normals by two Box-Muller transforms, (word 0, word 1) -> r cos t, r sin t and (word 2, word 3) likewise,
              r = sqrt(-2 ln u01(.)), t = 2 pi u01(.); element 4 q + j is the j-th of them times std
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
NOISE_DOMAIN, MASK_DOMAIN = 0x5EED, 0xD60B
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Counter words and key words as uint64 arrays (or scalars) holding 32-bit values; returns the four output words likewise."""
    c0, c1, c2, c3 = (_u64(c) & _LO for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for r in range(rounds):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)                   # < 2^64: no wrap
        kk0, kk1 = np.uint64((k0 + r * W0) & 0xFFFFFFFF), np.uint64((k1 + r * W1) & 0xFFFFFFFF)
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ kk0, p1 & _LO, (p0 >> _S32) ^ c3 ^ kk1, p0 & _LO
    return c0, c1, c2, c3


def u01(x):
    """float32, in the kernel's operation order: convert (exact, < 2^24), add one half (rounds to even from 2^23 on), scale (exact)."""
    return ((_u64(x) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def _words(count, seed, offset, domain, rounds=10, swap13=False, drop_high=False):
    """The four output words of counters offset .. offset + count - 1.  rounds / swap13 / drop_high: the deliberately broken variants of
    tests/test_rng_host.py (nine rounds; output words 1 and 3 exchanged; the counter's high word left at zero)."""
    with np.errstate(over='ignore'):
        ctr = np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(count, dtype=np.uint64)          # wraps at 2^64 like the device's
    hi = np.zeros_like(ctr) if drop_high else ctr >> _S32
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(ctr & _LO, hi, np.uint64(domain), np.uint64(0), seed & 0xFFFFFFFF, seed >> 32, rounds)
    return (w[0], w[3], w[2], w[1]) if swap13 else w


def dropout_keep(n, rate, seed, offset, **broken):
    """Boolean [n]: True where the element is kept."""
    return ~(u01(_words(n, seed, offset, MASK_DOMAIN, **broken)[0]) < np.float32(rate))


def dropout_mask(n, rate, seed, offset, **broken):
    """float32 [n]: 0 where dropped, float32(1) / (float32(1) - float32(rate)) where kept."""
    kept = np.float32(1) / (np.float32(1) - np.float32(rate))
    return np.where(dropout_keep(n, rate, seed, offset, **broken), kept, np.float32(0)).astype(np.float32)


def randn(n, std, seed, offset, **broken):
    """float64 [n]: std times the normals of counters offset .. offset + ceil(n / 4) - 1, from the float32 uniforms, everything after
    them in float64 (the device computes in fp32 with fast intrinsics and rounds once to bf16: see tests/test_gpu_rng.py for the bound)."""
    nq = (n + 3) // 4
    w = _words(nq, seed, offset, NOISE_DOMAIN, **broken)
    u = [u01(x).astype(np.float64) for x in w]
    out = np.empty((nq, 4), dtype=np.float64)
    for pair in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[2 * pair]))
        t = 2.0 * np.pi * u[2 * pair + 1]
        out[:, 2 * pair], out[:, 2 * pair + 1] = r * np.cos(t), r * np.sin(t)
    return float(std) * out.reshape(-1)[:n]


# ---- the two large cases both test modules use: more quads / elements than the 8192 x 256 threads of the largest grid (so the grid-stride
# loop runs), an offset whose low word carries into the high word inside the range, and (noise) an n % 4 = 3 tail ----
GRID_THREADS = 8192 * 256
BIG_NOISE = dict(n=4 * GRID_THREADS + 12003, seed=1234, offset=2 ** 32 - 12345)
BIG_MASK = dict(n=GRID_THREADS + 1000, rate=0.2, seed=(0x9E3779B9 << 32) | 99, offset=2 ** 32 - 777)
A_CAP = 2.0 ** -6                # the most the device's fast log / sin / cos may cost, in units of std (tests/test_gpu_rng.py)


def noise_excess(got, ref, std):
    """(|got - ref| - 2^-8 |ref|) / std per element: what is left of the error once one rounding to bf16 is taken out (8 significant
    bits: round-to-nearest errs by at most 2^-8 relative, half a unit in the last place at the bottom of a binade), in units of the
    standard deviation.  The device passes where this is <= A everywhere."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return (np.abs(got - ref) - 2.0 ** -8 * np.abs(ref)) / std


# ---- the statistics that tests/test_rng_host.py bounds for the restatement and tests/test_gpu_rng.py for the device ----
P_ABS_GT3 = 0.0026998            # P(|z| > 3) of a standard normal
MAX_ABS = float(np.sqrt(2 * 25 * np.log(2)))      # u01 >= 2^-25  ->  r <= sqrt(50 ln 2) = 5.887


def noise_statistics(z):
    """z: float64 [n] standard-normal candidates in stream order.  Returns name -> (value, standard error) for every bounded statistic;
    a statistic passes where |value| <= 5 standard errors.  (max|z| is bounded separately: it is a hard limit, not a statistic.)"""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    se = 1.0 / np.sqrt(n)
    st = {
        'mean': (z.mean(), se),
        'var - 1': ((z * z).mean() - 1.0, np.sqrt(2.0) * se),
        'E z^3': ((z ** 3).mean(), np.sqrt(15.0) * se),
        'E z^4 - 3': ((z ** 4).mean() - 3.0, np.sqrt(96.0) * se),
        'share(|z| > 3)': ((np.abs(z) > 3.0).mean() - P_ABS_GT3, np.sqrt(0.0027 / n)),
    }
    q = z[:n // 4 * 4].reshape(-1, 4)
    sq = 1.0 / np.sqrt(q.shape[0])
    c = np.corrcoef(q.T)
    for a in range(4):
        for b in range(a + 1, 4):
            st['corr(lane %d, lane %d)' % (a, b)] = (c[a, b], sq)
    st['lag-1 corr(lane 0)'] = (np.corrcoef(q[:-1, 0], q[1:, 0])[0, 1], sq)
    return st


def keep_statistic(keep, rate):
    """(keep share - (1 - rate), standard error) of a boolean mask."""
    keep = np.asarray(keep)
    return keep.mean() - (1.0 - rate), np.sqrt(rate * (1.0 - rate) / keep.size)
