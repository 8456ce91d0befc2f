"""CPU: the numpy restatement of the device RNG (tests/rng_restate.py) is Philox-4x32-10 (the published Random123 known answers), stays
inside every statistical bound that tests/test_gpu_rng.py puts on the device at that test's own sizes and offsets, and those checks are
not vacuous: a restatement broken in one of three ways leaves a bound or differs from the exact stream."""
import functools

import numpy as np
import pytest

import rng_restate as R

# Random123 kat_vectors, philox4x32 10: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(g) for g in got) == want, [hex(int(g)) for g in got]
    # vectorised: the same answer in every position of an array, next to another counter
    arr = R.philox4x32_10(*(np.array([c, 1, c], dtype=np.uint64) for c in ctr), *key)
    assert all(int(a[0]) == w and int(a[2]) == w for a, w in zip(arr, want))
    assert any(int(a[1]) != w for a, w in zip(arr, want))


def test_u01_is_the_kernels_float32_expression():
    x = np.array([0, 255, 256, 0x7fffff00, 0x80000000, 0x800000ff, 0xfffffe00, 0xffffffff], dtype=np.uint64)
    u = R.u01(x)
    assert u.dtype == np.float32
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)               # below 2^23 the half is kept
    assert u[4] == u[5] == np.float32(0.5)                                # 2^23 + 0.5 rounds to even: down
    assert u[6] == np.float32((2 ** 24 - 2) * 2.0 ** -24) and u[7] == np.float32(1.0)       # ties to even: 2^24 - 1.5 down, 2^24 - 0.5 up to 1
    assert u.min() > 0


@functools.lru_cache(maxsize=None)
def _big_noise(**broken):
    z = R.randn(R.BIG_NOISE['n'], 1.0, R.BIG_NOISE['seed'], R.BIG_NOISE['offset'], **broken)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _big_keep(**broken):
    k = R.dropout_keep(R.BIG_MASK['n'], R.BIG_MASK['rate'], R.BIG_MASK['seed'], R.BIG_MASK['offset'], **broken)
    k.setflags(write=False)
    return k


def test_restatement_meets_the_gpu_bounds():
    st = R.noise_statistics(_big_noise())
    for name, (v, se) in st.items():
        print('   %-22s %+.3e  = %+.2f se' % (name, v, v / se))
    assert len(st) == 12
    for name, (v, se) in st.items():
        assert abs(v) <= 5 * se, (name, v, se)
    assert np.abs(_big_noise()).max() <= R.MAX_ABS
    v, se = R.keep_statistic(_big_keep(), R.BIG_MASK['rate'])
    print('   %-22s %+.3e  = %+.2f se' % ('keep share - 0.8', v, v / se))
    assert abs(v) <= 5 * se


def test_mask_values_and_tail_of_the_restatement():
    m = R.dropout_mask(1000, 0.2, 7, 3)
    assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(0.2))}
    assert np.all(R.dropout_mask(1000, 0.0, 7, 3) == 1)                   # u01 > 0: rate 0 drops nothing
    # element 4 q + j comes from counter offset + q: a stream that starts one counter later is the same stream shifted by four
    a, b = R.randn(23, 0.5, 11, 2 ** 32 - 3), R.randn(19, 0.5, 11, 2 ** 32 - 2)
    assert np.array_equal(a[4:], b)
    # offset + i wraps at 2^64
    assert np.array_equal(R.dropout_keep(8, 0.5, 1, 2 ** 64 - 3)[3:], R.dropout_keep(5, 0.5, 1, 0))


BROKEN = {'nine rounds': dict(rounds=9), 'words 1 and 3 swapped': dict(swap13=True), 'high counter word dropped': dict(drop_high=True)}


@pytest.mark.parametrize('name', list(BROKEN))
def test_broken_restatement_is_caught(name):
    """Each mutant must be told from the true stream by a check the GPU test makes: the exact mask, or the elementwise noise bound at its
    cap A = 2^-6 (a mutant that is still a good generator passes the moment bounds, and may)."""
    kw = BROKEN[name]
    keep, bad_keep = _big_keep(), _big_keep(**kw)
    ref, bad = _big_noise(), _big_noise(**kw)
    miss = R.noise_excess(bad, ref, 1.0) > R.A_CAP
    carry_m, carry_n = 2 ** 32 - R.BIG_MASK['offset'], 4 * (2 ** 32 - R.BIG_NOISE['offset'])
    print('   %s: mask differs in %d of %d, noise outside the bound in %d of %d' % (name, int((keep != bad_keep).sum()), keep.size,
                                                                                     int(miss.sum()), miss.size))
    if name == 'words 1 and 3 swapped':
        assert np.array_equal(keep, bad_keep)                             # the mask reads word 0 only
        assert miss.mean() > 0.9
    elif name == 'high counter word dropped':
        # identical up to the carry, another stream after it: only a test that crosses 2^32 sees it
        assert np.array_equal(keep[:carry_m], bad_keep[:carry_m]) and not miss[:carry_n].any()
        assert (keep[carry_m:] != bad_keep[carry_m:]).mean() > 0.25 and miss[carry_n:].mean() > 0.9
    else:
        assert (keep != bad_keep).mean() > 0.25 and miss.mean() > 0.9
