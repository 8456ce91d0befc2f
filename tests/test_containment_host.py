"""CPU: the boundary search of tests/containment_cases.py, checked where it runs -- on the host, with the dry run of the dispatch.

For every gather K-split variant of the representative lists the smallest vg_conv_desc::scratch_bytes that keeps the variant equals
VG_SCRATCH_CTR_BYTES + cells * ks * one fp32 partial tile recomputed from vg_conv3d_plan, and the plan 16 bytes below has a smaller split;
for every conv_dma descriptor at N = 1, 2, 3 what vg_conv3d_scratch_bytes asks for keeps the roomy plan, the operand-only size drops the K
split and one byte less is refused; each weight-gradient family's plan changes one float below its boundary.  So the sizes at which
tests/test_gpu_containment.py launches are the library's boundaries, not the test's."""
import re

import pytest

import containment_cases as CC

_KS = CC.ksplit_cases()
_DMA = CC.dma_cases()


def test_counter_bytes_constant():
    from van_gan_amd import _lib
    assert CC.CTR == _lib.SCRATCH_CTR_BYTES
    text = open(__file__.replace('tests/test_containment_host.py', 'include/vangan_hip.h')).read()
    assert re.search(r'#define VG_SCRATCH_CTR_BYTES %d\b' % CC.CTR, text)


def test_case_lists_are_what_the_lists_hold():
    import layer_recipes as LR
    have = {kv for reps in (LR.representatives(), LR.inference_representatives(), LR.ragged_representatives(), LR.batch3_representatives())
            for kv in reps if kv[1].startswith('conv<') and CC.ks_of(kv[1]) >= 2}
    assert {(c['kind'], c['variant']) for c in _KS.values()} == have and len(have) >= 30
    assert {CC.ks_of(c['variant']) for c in _KS.values()} == {2, 3, 4, 6, 8}
    assert {c['kind'] for c in _KS.values()} == {'fwd', 'dgrad'}
    assert len(_DMA) % 3 == 0 and len(_DMA) >= 18
    assert set(CC.wgrad_cases()) >= {'wgrad_thin', 'wgrad_dma', 'wgrad_pw_dma', 'c1m_wgrad', 'wgrad'}


@pytest.mark.parametrize('cid', sorted(_KS))
def test_ksplit_boundary_is_the_plans_partial_tiles(cid):
    b = CC.ksplit_boundary(cid)
    ks = CC.ks_of(_KS[cid]['variant'])
    assert b['S'] == b['expected'], b
    assert (b['S'] - CC.CTR) % (ks * b['plan'][3]) == 0 and b['plan'][3] * ks <= 1024          # cells * ks slots, at most 1024 of them
    fam = lambda v: v.rsplit('|ks', 1)[0]
    assert fam(b['below']) == fam(_KS[cid]['variant']) and CC.ks_of(b['below']) < ks, b       # 16 bytes less: a smaller split or none
    assert fam(b['none']) == fam(_KS[cid]['variant']) and CC.ks_of(b['none']) == 1, b           # no workspace: no split


@pytest.mark.parametrize('cid', sorted(_DMA))
def test_conv_dma_boundaries(cid):
    b = CC.dma_boundary(cid)
    split = '|ks1|' in b['roomy']
    assert b['at_need'] == b['roomy'] and b['S'] <= b['need'], b               # what the query asks for runs the roomy plan
    assert b['below_floor'] is None and b['at_floor'] is not None, b         # below the operand: VG_EINVAL
    assert b['at_floor'] == b['roomy'].replace('|ks1|', '|ks0|'), b          # operand only: the same plan without the K split
    assert (b['floor'] - CC.CTR) % 256 == 0 and b['floor'] > CC.CTR
    if split:
        # need = counters + operand + units * ks partial tiles; S = the same with the smallest split, two slices: so the partial tiles of
        # the preferred plan are a whole number ks >= 2 of slices of (S - floor) / 2 bytes, whatever a tile's size is
        two = b['S'] - b['floor']
        assert two > 0 and two % 2 == 0 and b['need'] >= b['S'] and (b['need'] - b['floor']) % (two // 2) == 0, b
        assert b['below_S'] == b['at_floor'], b
    else:
        assert b['need'] == b['floor'] == b['S'], b


def test_conv_dma_operand_grows_with_the_batch():
    """The materialised operand is N samples of one size, rounded up to 256 bytes once."""
    by = {}
    for cid in _DMA:
        by.setdefault(cid.rsplit(' N', 1)[0], {})[int(cid.rsplit(' N', 1)[1])] = CC.dma_boundary(cid)['floor'] - CC.CTR
    for key, p in by.items():
        assert set(p) == {1, 2, 3}
        for n in (2, 3):
            assert 0 <= n * p[1] - p[n] < 256 * n, (key, p)


def test_weight_gradient_boundaries():
    for fam, c in CC.wgrad_cases().items():
        assert c['S'] % CC.WGRAD_GRANULE == 0 and 0 < c['S'] < CC.WGRAD_ROOMY
        assert c['below'] != c['roomy'] and c['none'] != c['roomy'], (fam, c['roomy'])
