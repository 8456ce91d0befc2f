"""CPU: every kernel variant, non-convolution regime and finalisation tail that a RAGGED patch selects has a parity case on the GPU
(tests/test_gpu_ragged.py).

tests/test_variant_coverage.py's argument, one step further: its walks are driven by 32^3, 64^3, 128x128x64 and 128^3, whose level grids
are powers of two on every axis, while the engine takes any patch with axes that are multiples of 16 and at least 32.  The train steps
of 32x48x80 (batch 1, batch 2) and 48x80x96 (batch 1) and the inference forwards of the same two windows select 133 (kind, variant)
pairs; 50 of them appear in no other walk of the suite, and the other 83 run their masked tile tails, odd class extents and last slabs
only here.  This file proves that the GPU module's case lists are those walks, that each case is a ragged call that selects exactly its
variant, and pins the ragged-only set BY NAME: a dispatch change that moves a ragged patch onto other kernels fails here and has to be
acknowledged."""
import pytest
import torch

import call_recipes as CR
import layer_recipes as LR
import test_gpu_ragged as TR


# what only the ragged walks select: no walk of layer_recipes.CONFIGS / INFER_CONFIGS launches these
RAGGED_ONLY = {
    'dgrad': {
        'conv32<128,1,n0,cp1>|walk0|ch1',
        'conv32<64,2,n0,cp0>|walk0|ch1',
        'conv32<64,4,n0,cp0>|walk0|ch0',
        'conv32<64,4,n0,cp0>|walk0|ch1',
        'conv<bf16,16,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks4',
        'conv<bf16,16,2,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks2',
        'conv<bf16,16,2,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks4',
        'conv<bf16,16,2,n0,wl0,dma0,mc1,c10>|walk0|ch0|ks1',
        'conv<bf16,16,4,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks2',
        'conv<bf16,16,4,n0,wl0,dma0,mc2,c10>|walk0|ch1|ks1',
        'conv<bf16,16,4,n0,wl1,dma0,mc1,c10>|walk0|ch0|ks1',
        'conv<bf16,32,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv<bf16,32,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks4',
        'conv<bf16,32,1,n0,wl1,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv<bf16,32,2,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks2',
        'conv<bf16,32,4,n0,wl0,dma0,mc2,c10>|walk0|ch1|ks1',
        'conv<bf16,64,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks2',
        'conv<bf16,64,1,n0,wl0,dma0,mc0,c11>|walk0|ch0|ks1',
        'conv<bf16,64,1,n0,wl0,dma0,mc2,c10>|walk0|ch1|ks1',
        'conv<bf16,64,2,n0,wl0,dma0,mc0,c10>|walk0|ch0|ks1',
        'conv<bf16,64,2,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv<bf16,64,2,n0,wl1,dma0,mc0,c10>|walk0|ch0|ks1',
        'conv<bf16,64,2,n0,wl1,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv_dma<64,256>|td2|gt9|nwb3|ks0|cls0|walk0|bs1',
        'conv_dma<64,256>|td8|gt8|nwb4|ks0|cls1|walk1|bs0',
        'conv_thin2<m0,b0,r0,s0>|walk0|ch1',
    },
    'fwd': {
        'conv<bf16,16,4,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks2',
        'conv<bf16,16,4,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks6',
        'conv<bf16,32,1,n0,wl0,dma0,mc0,c10>|walk0|ch0|ks1',
        'conv<bf16,32,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks3',
        'conv<bf16,32,1,n1,wl0,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv<bf16,32,2,n0,wl0,dma0,mc0,c10>|walk0|ch0|ks1',
        'conv<bf16,32,2,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks2',
        'conv<bf16,32,4,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv<bf16,32,4,n1,wl0,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv<bf16,64,2,n1,wl0,dma0,mc0,c10>|walk0|ch1|ks1',
        'conv_thin<m1,b1,r0,s1>|walk0|ch2',
    },
    'wgrad': {
        'wgrad<bf16,2,4,n0>|bm128|cib64|part1|walk0',
        'wgrad<bf16,24,1,n1>|bm256|cib32|part1|walk0',
        'wgrad<bf16,6,4,n1>|bm64|cib16|part0|walk1',
        'wgrad<bf16,6,4,n1>|bm64|cib16|part1|walk1',
        'wgrad<bf16,7,4,n0>|bm128|cib16|part1|walk0',
        'wgrad<bf16,7,4,n0>|bm128|cib16|part1|walk1',
        'wgrad<bf16,7,4,n0>|bm64|cib16|part1|walk0',
        'wgrad_dma<4,1,d0>|bm128|pl1|s1|nb5|part1|walk1',
        'wgrad_dma<4,1,d1>|bm128|pl1|s2|nb3|part1|walk1',
        'wgrad_dma<4,1,d1>|bm512|pl1|s1|nb3|part1|walk0',
        'wgrad_dma<4,2,d0>|bm128|pl1|s1|nb5|part1|walk1',
        'wgrad_dma<4,2,d0>|bm256|pl1|s1|nb4|part1|walk1',
        'wgrad_thin<m1>|ch0|walk0',
    },
}


def _walk_pairs():
    return {(k, v) for recs, _ in LR.all_ragged_walks().values() for k, _, v, _ in recs}


def _is_pow2(n):
    return n & (n - 1) == 0


def test_the_ragged_walks_are_the_ones_named():
    assert LR.RAGGED_CONFIGS == {'32x48x80 B1': ((32, 48, 80), 1), '32x48x80 B2': ((32, 48, 80), 2), '48x80x96 B1': ((48, 80, 96), 1)}
    assert sorted(LR.RAGGED_INFER_CONFIGS.values()) == [((32, 48, 80), 2), ((48, 80, 96), 1), ((48, 80, 96), 2)]
    walks = LR.all_ragged_walks()
    assert list(walks) == list(LR.RAGGED_CONFIGS) + list(LR.RAGGED_INFER_CONFIGS)
    for cfg in LR.RAGGED_CONFIGS:
        kinds = [k for k, _, _, _ in walks[cfg][0]]
        assert len(kinds) == 101 and kinds.count('fwd') == 34 and kinds.count('wgrad') == 34, cfg     # the whole step, as at 32^3
    for cfg in LR.RAGGED_INFER_CONFIGS:
        assert [k for k, _, _, _ in walks[cfg][0]] == ['fwd'] * 29 and [n for n, _ in walks[cfg][1]] == ['vg_stem_short_fwd'], cfg
    # the tables the other proofs are driven by are untouched
    assert set(LR.CONFIGS) == {'128^3 B1', '64^3 B2', '128x128x64 B2', '32^3 B1'} and not set(LR.CONFIGS) & set(LR.RAGGED_CONFIGS)
    assert len(LR.INFER_CONFIGS) == 4 and not set(LR.INFER_CONFIGS) & set(LR.RAGGED_INFER_CONFIGS)
    assert all(_is_pow2(n) for dims, _ in list(LR.CONFIGS.values()) + list(LR.INFER_CONFIGS.values()) for n in dims)


def test_every_variant_of_the_ragged_walks_has_a_gpu_parity_case():
    need = _walk_pairs()
    assert len(need) == 133
    reps = LR.ragged_representatives()
    assert set(reps) == need
    # the GPU module is parametrised over exactly these, none filtered out
    assert sorted(TR._KEYS) == sorted(need) and len(set(TR._KEYS)) == len(TR._KEYS)
    assert TR._REPS is reps
    marks = [m.name for m in TR.pytestmark] if isinstance(TR.pytestmark, list) else [TR.pytestmark.name]
    assert marks == ['gpu']


def test_every_representative_is_a_ragged_call_that_selects_exactly_its_variant():
    walks = LR.all_ragged_walks()
    for (kind, variant), r in LR.ragged_representatives().items():
        assert r['config'] in walks and r['recipe']['kind'] == kind
        # it IS a recorded call of that walk: the same recipe object, under that layer's name, with that variant
        assert any(rec is r['recipe'] and k == kind and v == variant and n == r['layer'] for k, n, v, rec in walks[r['config']][0]), (kind, variant)
        assert LR.replay_variant(r['recipe']) == variant, (kind, variant)       # the rebuilt call, dry: what run_recipe asserts before it launches
        grid = LR.out_grid(r['recipe'])
        assert any(not _is_pow2(n) for n in grid), (kind, variant, grid)
        assert r['macs'] <= 18.2e9                                      # nothing heavier than down2's data gradient at 48x80x96
    # no power-of-two call stands in for a ragged one
    pow2 = {id(rec) for recs in LR.all_records().values() for _, _, _, rec in recs}
    pow2 |= {id(rec) for recs, _ in LR.all_inference_walks().values() for _, _, _, rec in recs}
    assert not pow2 & {id(r['recipe']) for r in LR.ragged_representatives().values()}


def test_dry_run_of_every_recorded_ragged_call_is_stable():
    """The same call selects the same variant when the walk is repeated (the dispatch has no hidden state): the strings the cases
    assert are the strings a fresh walk reports, for all three kinds."""
    for cfg, (dims, B) in LR.RAGGED_CONFIGS.items():
        again = LR.walk_config(dims, B)
        assert [(k, n, v) for k, n, v, _ in again[0]] == [(k, n, v) for k, n, v, _ in LR.all_ragged_walks()[cfg][0]]
        assert again[1] == LR.all_ragged_walks()[cfg][1]
    for cfg, (dims, N) in LR.RAGGED_INFER_CONFIGS.items():
        h = LR.walk_inference(dims, N, torch.float16)                   # and the fp16 network walks the same strings
        assert [(k, n, v) for k, n, v, _ in h[0]] == [(k, n, v) for k, n, v, _ in LR.all_ragged_walks()[cfg][0]]


def test_the_grids_are_the_awkward_ones():
    grids = {LR.out_grid(r['recipe']) for r in LR.ragged_representatives().values()}
    extents = {n for g in grids for n in g}
    assert {3, 5} <= extents                                            # odd extents: the bridges 2x3x5 and 3x5x6
    assert {2, 4, 6} <= {n % 8 for n in extents}                        # and tails of 2, 4 and 6 behind a multiple of 8
    assert {(2, 3, 5), (3, 5, 6), (4, 6, 10), (6, 10, 12), (8, 12, 20), (12, 20, 24), (16, 24, 40), (24, 40, 48), (32, 48, 80), (48, 80, 96)} <= grids
    # strided data gradients that write an odd-extent class grid back to twice its size
    assert any(r['recipe']['kind'] == 'dgrad' and r['recipe']['layer']['stride'] == 2 and LR.out_grid(r['recipe']) in ((4, 6, 10), (6, 10, 12))
               for r in LR.ragged_representatives().values())


def test_ragged_only_variants_are_pinned_by_name():
    new = LR.ragged_only_variants()
    assert len(new) >= 40
    have = set(LR.representatives()) | set(LR.inference_representatives())
    assert not set(new) & have and set(new) == _walk_pairs() - have
    got = {kind: {v for k, v in new if k == kind} for kind in ('dgrad', 'fwd', 'wgrad')}
    for kind in got:
        assert got[kind] == RAGGED_ONLY[kind], (kind, sorted(got[kind] - RAGGED_ONLY[kind]), sorted(RAGGED_ONLY[kind] - got[kind]))
    assert [len(RAGGED_ONLY[k]) for k in ('dgrad', 'wgrad', 'fwd')] == [26, 13, 11]
    fams = {v.split('<')[0] for _, v in new}
    assert {'conv', 'conv32', 'conv_dma', 'conv_thin', 'conv_thin2', 'wgrad', 'wgrad_dma', 'wgrad_thin'} <= fams, fams
    assert TR._NEW == new


def test_fp16_cases_are_the_forward_variants_of_the_ragged_inference_walks():
    walks = LR.all_ragged_walks()
    need = {(k, v) for cfg in LR.RAGGED_INFER_CONFIGS for k, _, v, _ in walks[cfg][0]}
    reps = LR.ragged_inference_representatives()
    assert set(reps) == need and sorted(TR._IKEYS) == sorted(need) and len(need) >= 25
    for (kind, variant), r in reps.items():
        assert kind == 'fwd' and r['config'] in LR.RAGGED_INFER_CONFIGS and LR.recipe_variant(r['recipe']) == variant
        assert any(not _is_pow2(n) for n in LR.out_grid(r['recipe']))
    rs = [r['recipe'] for r in reps.values()]
    assert any(r['res'] and not r.get('res_c1') for r in rs) and any(r.get('res_c1') for r in rs)
    assert any(r['tanh'] and r['out_f32'] for r in rs) and any(r['sums'] for r in rs) and any(r['src']['shift0'] and r['src']['c1'] for r in rs)


def test_ksplit_stress_cases_are_the_selection_of_the_layer_suite():
    """tests/test_gpu_layers.py's _KSPLIT rule over the ragged-only variants: `conv<` forwards with more than one K slice (the ragged-only
    conv_dma data gradients have `|ks0|`: none qualifies), and the tails those forwards carry."""
    want = sorted(('fwd', v) for v in RAGGED_ONLY['fwd'] if v.startswith('conv<') and v.rsplit('|ks', 1)[-1] not in ('0', '1'))
    assert sorted(TR._KSPLIT) == want and {v.rsplit('|ks', 1)[-1] for _, v in want} == {'2', '3', '6'}
    assert not [v for v in RAGGED_ONLY['dgrad'] if v.startswith('conv_dma') and '|ks1|' in v]
    tails = {TR._CASES[cid]['variant'] for cid in TR._KSPLIT_FIN}
    assert tails == {v for _, v in want if any(t == v for t, _ in CR.ragged_needed_fin())} and tails


def test_every_ragged_call_regime_and_tail_has_a_gpu_case():
    cases = CR.ragged_call_cases()
    assert TR._CASES is cases and sorted(TR._CIDS) == sorted(cases)
    cov = {c for case in cases.values() for c in case['covers']}
    old = {c for case in CR.call_cases().values() for c in case['covers']}
    need = CR.ragged_needed_calls()
    missing = [c for c in need if c not in cov and c not in old]        # dropped only where call_cases() has the identical regime
    assert not missing, missing[:5]
    assert {n for n, _ in need} == {'vg_actnorm_bwd', 'vg_actnorm_bwd_stats', 'vg_actnorm_bwd_apply', 'vg_actnorm_bwd_apply2', 'vg_concat_bwd',
                                    'vg_stem_short_fwd', 'vg_stem_short_bwd', 'vg_tanh_bwd'}
    fin = CR.ragged_needed_fin()
    assert len(fin) >= 30 and not [k for k in fin if ('fin',) + k not in cov]           # no tail dropped: every one is a ragged call
    walks = LR.all_ragged_walks()
    for cid, c in cases.items():
        assert c['config'] in walks, cid
        if c['kind'] == 'fin':
            r = c['recipe']
            assert any(rec is r for _, _, _, rec in walks[c['config']][0]) and LR.recipe_variant(r) == c['variant'], cid
            assert CR.fin_shape(r) == c['covers'][0][2] and any(not _is_pow2(n) for n in LR.out_grid(r)), cid
            assert r['fin']['count'] == float(torch.tensor(LR.out_grid(r)).prod()), cid
        elif c['kind'] in ('anb', 'apply2'):
            r = dict(c['regime'] if c['kind'] == 'anb' else c['regime'][0][1])
            assert any(not _is_pow2(r[a]) for a in 'DHW'), cid
    kinds = {c['kind'] for c in cases.values()}
    assert kinds == {'anb', 'apply2', 'decoder', 'fin', 'stem_short_fwd', 'stem_short_bwd', 'tanh_bwd'}, kinds
    # the regimes the step depends on, at ragged grids
    anb = [dict(c['regime']) for c in cases.values() if c['kind'] == 'anb']
    assert any(r['alias_n0'] > 0 and 0 < r['pgrad_n'] < r['N'] for r in anb) and any(r['has_mult'] and r['act'] == 2 for r in anb)
    assert any(r['has_x1'] and r['x0_shift'] for r in anb) and any(r['accumulate'] for r in anb)
    assert any(r['g_padded'] and min(r['D'], r['H'], r['W']) in (2, 3) for r in anb)     # the double mirror at the bridges


def test_decoder_blocks_of_the_ragged_configs_match_the_walks():
    """dec0 and dec1 on the fused split kernel, dec2 and dec3 on the fall-back with vg_concat_bwd, at every ragged train config."""
    cases = CR.ragged_call_cases()
    for cfg in LR.RAGGED_CONFIGS:
        walk = sorted(tuple(v for k, v in r if k in ('N', 'D', 'H', 'W', 'Cu', 'Cs')) for n, r in LR.all_ragged_walks()[cfg][1] if n == 'vg_concat_bwd')
        blocks = CR.decoder_blocks(cfg, LR.RAGGED_CONFIGS)
        assert walk == sorted((b['N'], *b['dims'], b['c_low'], b['c_skip']) for b in blocks), cfg
        assert [(b['block'], b['served']) for b in blocks] == [('dec0', True), ('dec1', True), ('dec2', False), ('dec3', False)]
        for b in blocks:
            assert cases['decoder %s %s' % (b['block'], cfg)]['block'] == b and all(n % 2 == 0 for n in b['dims'])


def test_the_existing_case_lists_are_unchanged():
    """Nothing of this moved what tests/test_gpu_layers.py, test_gpu_infer_layers.py and test_gpu_calls.py run."""
    assert len(LR.representatives()) == len({(k, v) for recs in LR.all_records().values() for k, _, v, _ in recs}) == 154
    assert len(LR.inference_representatives()) == 44 and len(CR.call_cases()) == 137 and len(CR.inference_fin_cases()) == 8
    assert all(r['config'] in LR.CONFIGS for r in LR.representatives().values())
    assert all(r['config'] in LR.CONFIGS or r['config'] in LR.INFER_CONFIGS for r in LR.inference_representatives().values())
    assert all(c['config'] in LR.NEEDED for c in CR.call_cases().values())
    shared = set(CR.call_cases()) & set(CR.ragged_call_cases())         # ids carry the grid (decoder blocks: the config) -- except the tails'
    assert all(CR.call_cases()[cid]['kind'] == 'fin' and CR.ragged_call_cases()[cid]['recipe'] is not CR.call_cases()[cid]['recipe'] for cid in shared)
    assert CR.decoder_blocks('64^3 B2') == CR.decoder_blocks('64^3 B2', LR.CONFIGS)


def test_the_bounds_hold_for_the_reference_alone_on_a_ragged_grid():
    """The bounds of run_recipe do not depend on the grid: identical 16-bit operands, fp32 accumulation, one output rounding.  Here the
    reference itself is held to the forward bounds on a ragged call -- dec3.cb1 of the 32x48x80 walk (768 -> 256 channels on 4x6x10
    through the virtual upsample + concat, 20736-term sums, six K slices on the device): a float32 convolution of the rounded operands
    followed by the output rounding, against float64, for both storage types."""
    from oracle import vangan_oracle as O
    recipe = next(r for _, n, _, r in LR.all_ragged_walks()['infer 32x48x80 N2'][0] if n == 'dec3.cb1.conv')
    L, sr = recipe['layer'], recipe['src']
    assert tuple(sr['dims']) == (4, 6, 10) and sr['shift0'] == 1 and sr['c1'] > 0
    for st16 in (torch.bfloat16, torch.float16):
        g = torch.Generator().manual_seed(1)
        st, _ = LR.make_layer_from(L, 'cpu', dtype=st16)
        _, host = LR.make_operand(sr, L['pad'], 'cpu', g, st16)
        tol = LR.FWD_TOL[st16]
        ys = {}
        for dt in (torch.float64, torch.float32):
            ap = LR.ref_operand(sr, host, L['pad'], dt, st16)
            w = LR.bf(st.param('c.w').to(dt), st16)
            ys[dt] = O.to_ndhwc(O.conv3d(ap, w, st.param('c.b').to(dt) if L['bias'] else None, L['stride'], 'valid' if L['pad'] == 'reflect' else 'same'))
        got, ref = ys[torch.float32].to(st16), ys[torch.float64]
        assert got.shape[1:4] == (4, 6, 10)
        LR.close_bf16(got, ref, 'float32 reference + output rounding', rel=tol['rel'], floor=tol['floor'])
        sums = lambda y: torch.stack([y.sum(dim=(1, 2, 3)), (y ** 2).sum(dim=(1, 2, 3))], dim=-1)
        assert LR.rel_l2(sums(got.float()), sums(LR.bf(ref, st16))) < tol['sums']
