"""GPU parity at RAGGED patches: the kernels that legal patch sizes with no power-of-two level grids select, and the partial-tile paths
of the familiar ones.

ResUNet and PatchGAN take any patch whose axes are multiples of 16 and at least 32; every other shape-dependent proof of the suite is
driven by 32^3, 64^3, 128x128x64 and 128^3, whose level grids every tile divides.  Here the train steps of 32x48x80 (batch 1 and 2) and
48x80x96 (batch 1) and the inference forwards of the same two windows are walked in dry-run mode (layer_recipes.RAGGED_CONFIGS /
RAGGED_INFER_CONFIGS; level grids 16x24x40, 8x12x20, 4x6x10, 2x3x5 and 24x40x48, 12x20x24, 6x10x12, 3x5x6), and

  - every (kind, variant) of those walks -- 133, of which 50 have no case anywhere else (tests/test_ragged_coverage.py pins them by
    name) -- is replayed at the cheapest RAGGED call that selects it, as recorded, against the oracle's convolution / autograd on the
    same 16-bit-rounded operands (layer_recipes.run_recipe, its bounds unchanged: they follow from identical operands, fp32
    accumulation and one output rounding, not from the grid);
  - every forward variant of the ragged inference walks again on the fp16 library (FWD_TOL[torch.float16]);
  - every InstanceNorm-backward regime, two-job apply, decoder block (dec0 / dec1 on the fused split kernel, dec2 / dec3 on the
    fall-back with vg_concat_bwd), stem shortcut, tanh backward and (forward variant, tail job shape) of the walks through the
    replays of tests/test_gpu_calls.py (call_recipes.ragged_call_cases);
  - the K-split forwards among the 50 (|ks2, |ks3, |ks6) bitwise over 200 launches on two streams, their tails under the same load.

Masked tile tails, the class extents of strided data gradients on odd grids (3x5x6 -> 6x10x12), the last slab of a weight gradient and a
walker's last tile run here at these kernels' sizes.

What these cases found: every value inside its bound at the first run, and one address bug -- the staging
routines of vg_gather.h read the dummy of an out-of-grid halo column of the concat's SECOND source at src0's base plus src1's plane
offset, up to a src1 sample behind the four times smaller src0 (dec3.short's weight gradient at 4x6x10: 61 456 bytes into a 30 720-byte
tensor).  Masked afterwards, so no value can show it: only the whole suite's allocator layout made it fault.  Fixed in vg_gather.h.

Measured on an MI355X (325 cases, 22.5 s; the table is in DESIGN.md section 4):
  bf16 library, 41 forwards with a 16-bit output        max |err| / max |ref| 1.9e-3 .. 3.6e-3   statistics 2.9e-8 .. 1.7e-5
  bf16 library, 52 data gradients                       max |err| / max |ref| 1.9e-3 .. 3.8e-3
  bf16 library, 38 weight / 34 bias gradients           rel-L2 <= 3.7e-5 / <= 7.2e-7 (bound 2e-3)
  fp16 library, 30 forwards with a 16-bit output        2.4e-4 .. 4.3e-4 (half an fp16 ulp at max |ref|: 4.9e-4)   statistics <= 3.1e-6
  InstanceNorm backward, 67 regimes + 15 two-job applies  sums and gamma / beta gradients <= 3.4e-7 (bound 1e-4), bf16 dx <= 3.5e-3
  48 finalisation tails; 5 under load                   4.5e-8 .. 4.3e-7; <= 2.8e-7 (bound 1e-4)"""
import pytest
import torch

import call_recipes as CR
import layer_recipes as LR
import test_gpu_calls as TC

pytestmark = pytest.mark.gpu

_REPS = LR.ragged_representatives()
_KEYS = sorted(_REPS, key=lambda kv: (_REPS[kv]['macs'], kv))
_NEW = LR.ragged_only_variants()
_IREPS = LR.ragged_inference_representatives()
_IKEYS = sorted(_IREPS, key=lambda kv: (_IREPS[kv]['macs'], kv))
_CASES = CR.ragged_call_cases()
_CIDS = sorted(_CASES, key=lambda k: (_CASES[k]['kind'], k))


def _dev():
    return torch.device('cuda:0')


def _id(kv, reps=_REPS):
    r = reps[kv]
    return '%s %s [%s %s]' % (kv[0], kv[1], r['config'], r['layer'])


def _report(name, err):
    print('%-120s %s' % (name, '  '.join('%s %.2e' % kv for kv in sorted((err or {}).items()))))


# ----------------------------------------------------------------------------------------------------------------------
# convolution launches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kv', _KEYS, ids=[_id(kv) for kv in _KEYS])
def test_ragged_variant_matches_oracle(kv):
    """run_recipe asserts that the dry run of the rebuilt call selects exactly kv[1] before it launches."""
    err = LR.run_recipe(_REPS[kv]['recipe'], kv[1], _dev(), arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))
    _report('bf16 ' + _id(kv), err)


@pytest.mark.parametrize('kv', _IKEYS, ids=[_id(kv, _IREPS) for kv in _IKEYS])
def test_fp16_build_ragged_inference_variant_matches_oracle(kv):
    from van_gan_amd import ops
    with ops.Fp16():
        assert ops.lib.vg_storage16() == 1
        err = LR.run_recipe(_IREPS[kv]['recipe'], kv[1], _dev(), storage=torch.float16, arena=LR.guarded_for(_IREPS[kv]['recipe'], _dev()))
    _report('fp16 ' + _id(kv, _IREPS), err)


# the selection of tests/test_gpu_layers.py's _KSPLIT, over the ragged-only variants
_KSPLIT = [kv for kv in _NEW if (kv[1].startswith('conv_dma') and '|ks1|' in kv[1] and kv[0] == 'dgrad' and not _REPS[kv]['recipe']['accumulate']
                                 and not _REPS[kv]['recipe'].get('bstat'))
           or (kv[1].startswith('conv<') and kv[1].rsplit('|ks', 1)[-1] not in ('0', '1') and kv[0] == 'fwd')]
_KSPLIT_FIN = [cid for cid in _CIDS if _CASES[cid]['kind'] == 'fin' and ('fwd', _CASES[cid]['variant']) in _KSPLIT]


@pytest.mark.parametrize('kv', _KSPLIT, ids=[_id(kv) for kv in _KSPLIT])
def test_ragged_ksplit_exchange_is_bitwise_stable_under_load(kv):
    """The K slices' partial tiles of a ragged grid's last, partly masked tile go through the same per-stream scratch: 200 launches on two
    streams must reproduce the first bit for bit (tests/test_gpu_layers.py has the argument)."""
    LR.stress_recipe(_REPS[kv]['recipe'], kv[1], _dev(), launches=200, arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))


@pytest.mark.parametrize('cid', _KSPLIT_FIN)
def test_ragged_ksplit_finalisation_tail_under_load(cid):
    c = _CASES[cid]
    w = CR.stress_fin(c['recipe'], c['variant'], _dev(), launches=200, arena=LR.guarded_for(c['recipe'], _dev()))
    _report('fin under load ' + cid, dict(worst=w))


# ----------------------------------------------------------------------------------------------------------------------
# non-convolution calls and finalisation tails
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', _CIDS)
def test_ragged_recorded_call_matches_float64(cid):
    TC.run_case(_CASES[cid], cid, _dev())
