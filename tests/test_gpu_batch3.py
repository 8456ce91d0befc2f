"""GPU parity at BATCH 3, the reference's own per-GPU training batch (128^3 patches, three per GPU).

Every other shape-dependent proof of the suite runs a per-replica batch of 1 or 2: the generator's kernels see N in {1, 2, 4}, the
discriminator's N in {2, 3, 4, 6}.  At batch 3 the generator runs at N = 3 and 6, the discriminator at N = 6 and 9 (backward_both's
3B launch) -- no other call of the suite has N = 9, and no generator-side kernel is launched anywhere else with an N that is no power
of two.  N moves the host dispatch (workgroups against 256 CUs: K splits, conv_dma grid classes, weight-gradient slab plans, tile
walkers), the grids sized as cap / N with odd caps (767 / N, 511 / N, 2047 / N, 256 * per_cu / N) and their striped reductions, and the
alias arithmetic of the 2B + B discriminator sweep.  Here the train steps of 32^3, 64^3, 128x128x64, 128^3 and 32x48x80 at batch 3 are
walked in dry-run mode (layer_recipes.BATCH3_CONFIGS), and

  - every (kind, variant) of those walks -- 173, of which 23 have no case anywhere else (tests/test_batch3_coverage.py pins them by
    name) -- is replayed at the cheapest BATCH-3 call that selects it, N = 3, 6 or 9 as recorded, against the oracle's convolution /
    autograd on the same 16-bit-rounded operands (layer_recipes.run_recipe, its bounds unchanged: they follow from identical operands,
    fp32 accumulation and one output rounding, not from N);
  - every InstanceNorm-backward regime, two-job apply, decoder block, stem shortcut, tanh backward and (forward variant, tail job
    shape) of the walks through the replays of tests/test_gpu_calls.py (call_recipes.batch3_call_cases);
  - the K-split forwards among the 23 (|ks3, |ks4) bitwise over 200 launches on two streams, their tails under the same load.

No case is heavier than the heaviest one of tests/test_gpu_layers.py (103 GMAC) but one: down2's 9-sample data gradient at 128^3
(309 GMAC), whose variant no cheaper call selects (tests/test_batch3_coverage.py has the search); down0's (155 GMAC) runs with one axis
halved, where the dry run reports the identical variant (layer_recipes.shrink_call: the batch is never touched).

What these cases found: every value inside its bound at the first run, no address error, no dry run refused.

Measured on an MI355X (411 cases, 22.4 s; the table is in DESIGN.md section 4):
  55 forwards with a bf16 output                        max |err| / max |ref| 1.7e-3 .. 3.6e-3   statistics 1.3e-8 .. 2.2e-5
  56 data gradients                                     max |err| / max |ref| 2.0e-3 .. 3.8e-3
  57 weight / 51 bias gradients                         rel-L2 <= 3.0e-5 / <= 5.1e-7 (bound 2e-3)
  InstanceNorm backward, 108 regimes + 25 two-job applies  sums and gamma / beta gradients <= 6.3e-7 (bound 1e-4), bf16 dx <= 3.6e-3
  67 finalisation tails; 1 under load                   4.4e-8 .. 3.4e-7; 1.7e-7 (bound 1e-4)"""
import pytest
import torch

import call_recipes as CR
import layer_recipes as LR
import test_gpu_calls as TC

pytestmark = pytest.mark.gpu

_REPS = LR.batch3_representatives()
_KEYS = sorted(_REPS, key=lambda kv: (_REPS[kv]['macs'], kv))
_NEW = LR.batch3_only_variants()
_CASES = CR.batch3_call_cases()
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
def test_batch3_variant_matches_oracle(kv):
    """run_recipe asserts that the dry run of the rebuilt call selects exactly kv[1] before it launches."""
    err = LR.run_recipe(_REPS[kv]['recipe'], kv[1], _dev(), arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))
    _report('bf16 N%d ' % LR.recipe_n(_REPS[kv]['recipe']) + _id(kv), err)


# the selection of tests/test_gpu_layers.py's _KSPLIT, over the batch-3-only variants
_KSPLIT = [kv for kv in _NEW if (kv[1].startswith('conv_dma') and '|ks1|' in kv[1] and kv[0] == 'dgrad' and not _REPS[kv]['recipe']['accumulate']
                                 and not _REPS[kv]['recipe'].get('bstat'))
           or (kv[1].startswith('conv<') and kv[1].rsplit('|ks', 1)[-1] not in ('0', '1') and kv[0] == 'fwd')]
_KSPLIT_FIN = [cid for cid in _CIDS if _CASES[cid]['kind'] == 'fin' and ('fwd', _CASES[cid]['variant']) in _KSPLIT]


@pytest.mark.parametrize('kv', _KSPLIT, ids=[_id(kv) for kv in _KSPLIT])
def test_batch3_ksplit_exchange_is_bitwise_stable_under_load(kv):
    """The K slices' partial tiles of three samples go through the same per-stream scratch: 200 launches on two streams must reproduce
    the first bit for bit (tests/test_gpu_layers.py has the argument)."""
    LR.stress_recipe(_REPS[kv]['recipe'], kv[1], _dev(), launches=200, arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))


@pytest.mark.parametrize('cid', _KSPLIT_FIN)
def test_batch3_ksplit_finalisation_tail_under_load(cid):
    c = _CASES[cid]
    w = CR.stress_fin(c['recipe'], c['variant'], _dev(), launches=200, arena=LR.guarded_for(c['recipe'], _dev()))
    _report('fin under load ' + cid, dict(worst=w))


# ----------------------------------------------------------------------------------------------------------------------
# non-convolution calls and finalisation tails
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', _CIDS)
def test_batch3_recorded_call_matches_float64(cid):
    TC.run_case(_CASES[cid], cid, _dev())
