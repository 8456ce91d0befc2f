"""CPU: every kernel variant, non-convolution regime and finalisation tail that a train step at BATCH 3 selects has a parity case on the
GPU (tests/test_gpu_batch3.py).

tests/test_variant_coverage.py's argument along the batch axis.  The reference trains with three 128^3 patches per GPU (BASELINE.md
section 1); every other walk of the suite has a per-replica batch of 1 or 2, so the generator's kernels run at N in {1, 2, 4} and the
discriminator's at N in {2, 3, 4, 6}.  At batch 3 they run at N = 3 and 6, and at N = 6 and 9.  The train steps of 32^3, 64^3,
128x128x64, 128^3 and 32x48x80 at batch 3 select 173 (kind, variant) pairs; 23 of them appear in no other walk of the suite, and the
other 150 run other tile walks, last slabs, K-slice counts and cap / N grids here than anywhere else.  This file proves that the GPU
module's case lists are those walks, that each case is a batch-3 call (N = 3, 6 or 9) that selects exactly its variant, and pins the
batch-3-only set BY NAME: a dispatch change that moves the reference's own configuration onto other kernels fails here and has to be
acknowledged."""
import itertools
import math

import call_recipes as CR
import layer_recipes as LR
import test_gpu_batch3 as TB


# what only the batch-3 walks select: no walk of layer_recipes.CONFIGS / INFER_CONFIGS / RAGGED_CONFIGS / RAGGED_INFER_CONFIGS launches these
BATCH3_ONLY = {
    'dgrad': {
        'conv32<128,2,n0,cp0>|walk0|ch1',                               # dec3.short at 128x128x64
        'conv32<128,2,n0,cp0>|walk1|ch1',                               # dec3.short at 128^3
        'conv32<64,2,n0,cp1>|walk0|ch1',
        'conv<bf16,32,4,n0,wl0,dma0,mc0,c10>|walk1|ch0|ks1',
        'conv<bf16,32,4,n0,wl1,dma0,mc0,c11>|walk0|ch0|ks1',
        'conv<bf16,64,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks4',
        'conv<bf16,64,1,n0,wl1,dma0,mc0,c10>|walk0|ch0|ks1',
        'conv_dma<128,256>|td2|gt9|nwb2|ks0|cls0|walk1|bs1',            # dec3.cb1 at 128^3, N = 6
        'conv_dma<128,256>|td4|gt8|nwb2|ks0|cls0|walk1|bs0',            # down2 at 128^3, N = 9
    },
    'fwd': {
        'conv32<128,1,n1,cp0>|walk1|ch1',                               # down0 at 64^3, N = 6
        'conv<bf16,16,1,n1,wl0,dma0,mc0,c10>|walk0|ch1|ks4',            # the discriminator's 16-channel head at 128x128x64 ...
        'conv<bf16,16,2,n1,wl0,dma0,mc0,c10>|walk0|ch1|ks4',            # ... and at 128^3
        'conv<bf16,16,4,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks3',
    },
    'wgrad': {
        'wgrad<bf16,2,4,n0>|bm128|cib64|part1|walk1',
        'wgrad_dma<4,1,d0>|bm256|pl1|s1|nb5|part1|walk0',
        'wgrad_dma<4,1,d0>|bm256|pl1|s1|nb5|part1|walk1',
        'wgrad_dma<4,1,d1>|bm128|pl1|s2|nb3|part1|walk0',
        'wgrad_dma<4,1,d1>|bm256|pl1|s1|nb5|part1|walk1',
        'wgrad_dma<4,1,d1>|bm64|pl1|s2|nb5|part1|walk1',
        'wgrad_dma<8,1,d0>|bm128|pl1|s2|nb2|part1|walk1',
        'wgrad_dma<8,2,d0>|bm256|pl2|s1|nb2|part1|walk1',               # dec3.cb1 at 128x128x64
        'wgrad_pw_dma<4,4>|bm256|rs1|s2|u0|nb3|walk1',
        'wgrad_pw_dma<6,4>|bm64|rs4|s1|u1|nb2|walk1',
    },
}

# The one representative above the cost cap (103 GMAC, the heaviest case of tests/test_gpu_layers.py): down2's data gradient over the
# 9 samples of backward_both at 128^3, 256 <- 512 channels, 4^3 taps, on 16^3.  Its variant is the LDS-DMA kernel WITHOUT a K split
# (|ks0|) on the tile walker: the dispatch takes it only when the tiles alone fill the 256 CUs, so every cheaper call of the layer falls
# back to |ks1|walk0 (the B = 1 step's 3-sample call) or to another family.  test_the_case_above_the_cap_cannot_be_made_cheaper searches
# the grids; the recorded call stays, 309 GMAC.
ABOVE_CAP = {('dgrad', 'conv_dma<128,256>|td4|gt8|nwb2|ks0|cls0|walk1|bs0'): 309.3e9}


def _walk_pairs():
    return {(k, v) for recs, _ in LR.all_batch3_walks().values() for k, _, v, _ in recs}


def _older_pairs():
    old = {(k, v) for recs in LR.all_records().values() for k, _, v, _ in recs}
    old |= {(k, v) for recs, _ in LR.all_inference_walks().values() for k, _, v, _ in recs}
    return old | {(k, v) for recs, _ in LR.all_ragged_walks().values() for k, _, v, _ in recs}


def test_the_batch3_walks_are_the_ones_named():
    assert LR.BATCH3_CONFIGS == {'32^3 B3': ((32, 32, 32), 3), '64^3 B3': ((64, 64, 64), 3), '128x128x64 B3': ((128, 128, 64), 3),
                                 '128^3 B3': ((128, 128, 128), 3), '32x48x80 B3': ((32, 48, 80), 3)}
    walks = LR.all_batch3_walks()
    assert list(walks) == list(LR.BATCH3_CONFIGS)
    for cfg in LR.BATCH3_CONFIGS:
        kinds = [k for k, _, _, _ in walks[cfg][0]]
        assert len(kinds) == 101 and kinds.count('fwd') == 34 and kinds.count('wgrad') == 34, cfg     # the whole step, as at 32^3
        # the generator at N = 3 (forward) and 6 (paired backward sweep), the discriminator at 6 (forward) and 9 (backward_both)
        assert {LR.recipe_n(r) for _, _, _, r in walks[cfg][0]} == set(LR.BATCH3_N), cfg
    # the tables the other proofs are driven by are untouched, and no walk of theirs has a batch of three
    tables = (LR.CONFIGS, LR.INFER_CONFIGS, LR.RAGGED_CONFIGS, LR.RAGGED_INFER_CONFIGS)
    assert not any(set(LR.BATCH3_CONFIGS) & set(t) for t in tables)
    assert {B for t in tables for _, B in t.values()} == {1, 2}
    assert {d for d, _ in LR.BATCH3_CONFIGS.values()} == {d for d, _ in LR.CONFIGS.values()} | {(32, 48, 80)}


def test_every_variant_of_the_batch3_walks_has_a_gpu_parity_case():
    need = _walk_pairs()
    assert len(need) == 173
    reps = LR.batch3_representatives()
    assert set(reps) == need
    # the GPU module is parametrised over exactly these, none filtered out
    assert sorted(TB._KEYS) == sorted(need) and len(set(TB._KEYS)) == len(TB._KEYS)
    assert TB._REPS is reps
    marks = [m.name for m in TB.pytestmark] if isinstance(TB.pytestmark, list) else [TB.pytestmark.name]
    assert marks == ['gpu']


def test_every_representative_is_a_batch3_call_that_selects_exactly_its_variant():
    walks = LR.all_batch3_walks()
    cap = LR.macs_cap()
    assert 103.0e9 < cap < 103.1e9                                      # down2's data gradient at 128^3 B1
    over = {}
    for (kind, variant), r in LR.batch3_representatives().items():
        rec = r.get('recorded', r['recipe'])
        assert r['config'] in walks and r['recipe']['kind'] == kind
        # it IS a recorded call of that walk: the same recipe object, under that layer's name, with that variant
        assert any(x is rec and k == kind and v == variant and n == r['layer'] for k, n, v, x in walks[r['config']][0]), (kind, variant)
        assert LR.replay_variant(r['recipe']) == variant, (kind, variant)       # the rebuilt call, dry: what run_recipe asserts before it launches
        assert LR.recipe_n(r['recipe']) in LR.BATCH3_N and LR.recipe_n(r['recipe']) == LR.recipe_n(rec), (kind, variant)
        assert r['macs'] == LR.recipe_macs(r['recipe'])
        if r.get('shrunk'):                                             # axes halved, nothing else: the same layer, samples and flags
            assert LR.recipe_macs(rec) > cap >= r['macs']
            strip = lambda q: {k: ({a: b for a, b in v.items() if a not in ('in_dims', 'dims')} if isinstance(v, dict) else v)
                               for k, v in q.items() if k != 'fin'}
            assert strip(r['recipe']) == strip(rec), (kind, variant)
        if r['macs'] > cap:
            over[(kind, variant)] = r['macs']
    assert set(over) == set(ABOVE_CAP) and all(abs(over[k] - ABOVE_CAP[k]) < 1e8 for k in over), over
    # no call of an older walk stands in for a batch-3 one
    older = {id(rec) for recs in LR.all_records().values() for _, _, _, rec in recs}
    older |= {id(rec) for w in (LR.all_inference_walks(), LR.all_ragged_walks()) for recs, _ in w.values() for _, _, _, rec in recs}
    assert not older & {id(r.get('recorded', r['recipe'])) for r in LR.batch3_representatives().values()}
    # N = 9 is there: backward_both's sweep (no forward runs at 3B)
    n9 = {k for (k, _), r in LR.batch3_representatives().items() if LR.recipe_n(r['recipe']) == 9}
    assert 'dgrad' in n9 and 'fwd' not in n9, n9


def test_the_case_above_the_cap_cannot_be_made_cheaper():
    """Every call of down2's data gradient with 3, 6 or 9 samples on a grid with axes in 4 .. 24 (multiples of 4) that costs no more than
    the cap selects another variant; the cheapest that selects this one costs 290 GMAC, 6 % less than the recorded call."""
    (key, _), = ABOVE_CAP.items()
    r = LR.batch3_representatives()[key]
    assert not r.get('shrunk') and r['config'] == '128^3 B3' and r['layer'] == 'down2' and r['recipe']['N'] == 9
    assert LR.shrink_call(r['recipe'], key[1], LR.macs_cap()) is r['recipe']
    cheapest = None
    for N in LR.BATCH3_N:
        for d in itertools.combinations_with_replacement((4, 8, 12, 16, 20, 24), 3):
            cand = dict(r['recipe'], N=N, layer=dict(r['recipe']['layer'], in_dims=d))
            m = LR.recipe_macs(cand)
            if m >= r['macs']:
                continue
            try:
                same = LR.replay_variant(cand) == key[1]
            except Exception:
                same = False
            assert not (same and m <= LR.macs_cap()), (N, d, m)
            if same:
                cheapest = m if cheapest is None else min(cheapest, m)
    assert cheapest is not None and cheapest > 2.5 * LR.macs_cap(), cheapest


def test_dry_run_of_every_recorded_batch3_call_is_stable():
    """The same call selects the same variant when the walk is repeated (the dispatch has no hidden state): the strings the cases
    assert are the strings a fresh walk reports, for all three kinds."""
    for cfg, (dims, B) in LR.BATCH3_CONFIGS.items():
        again = LR.walk_config(dims, B)
        assert [(k, n, v) for k, n, v, _ in again[0]] == [(k, n, v) for k, n, v, _ in LR.all_batch3_walks()[cfg][0]]
        assert again[1] == LR.all_batch3_walks()[cfg][1]


def test_batch3_only_variants_are_pinned_by_name():
    new = LR.batch3_only_variants()
    assert len(new) == 23
    assert not set(new) & _older_pairs() and set(new) == _walk_pairs() - _older_pairs()
    got = {kind: {v for k, v in new if k == kind} for kind in ('dgrad', 'fwd', 'wgrad')}
    for kind in got:
        assert got[kind] == BATCH3_ONLY[kind], (kind, sorted(got[kind] - BATCH3_ONLY[kind]), sorted(BATCH3_ONLY[kind] - got[kind]))
    assert [len(BATCH3_ONLY[k]) for k in ('dgrad', 'wgrad', 'fwd')] == [9, 10, 4]
    fams = {v.split('<')[0] for _, v in new}
    assert {'conv', 'conv32', 'conv_dma', 'wgrad', 'wgrad_dma', 'wgrad_pw_dma'} <= fams, fams
    assert TB._NEW == new
    # where they come from: 20 of them from the power-of-two patches alone, 7 from the reference's own configuration
    walks = LR.all_batch3_walks()
    of = lambda cfgs: {(k, v) for cfg in cfgs for k, _, v, _ in walks[cfg][0]} & set(new)
    assert len(of([c for c in walks if c != '32x48x80 B3'])) == 20 and len(of(['128^3 B3'])) == 7
    assert len(of(['64^3 B3', '128x128x64 B3', '128^3 B3'])) == 11


def test_ksplit_stress_cases_are_the_selection_of_the_layer_suite():
    """tests/test_gpu_layers.py's _KSPLIT rule over the batch-3-only variants: `conv<` forwards with more than one K slice (the
    batch-3-only conv_dma data gradients have `|ks0|`: none qualifies), and the tails those forwards carry."""
    want = sorted(('fwd', v) for v in BATCH3_ONLY['fwd'] if v.startswith('conv<') and v.rsplit('|ks', 1)[-1] not in ('0', '1'))
    assert sorted(TB._KSPLIT) == want and {v.rsplit('|ks', 1)[-1] for _, v in want} == {'3', '4'}
    assert not [v for v in BATCH3_ONLY['dgrad'] if v.startswith('conv_dma') and '|ks1|' in v]
    tails = {TB._CASES[cid]['variant'] for cid in TB._KSPLIT_FIN}
    assert tails == {v for _, v in want if any(t == v for t, _ in CR.batch3_needed_fin())} and tails


def test_every_batch3_call_regime_and_tail_has_a_gpu_case():
    cases = CR.batch3_call_cases()
    assert TB._CASES is cases and sorted(TB._CIDS) == sorted(cases)
    cov = {c for case in cases.values() for c in case['covers']}
    old = {c for cs in (CR.call_cases(), CR.ragged_call_cases()) for case in cs.values() for c in case['covers']}
    need = CR.batch3_needed_calls()
    missing = [c for c in need if c not in cov and c not in old]        # dropped only where an older list has the identical regime
    assert not missing, missing[:5]
    assert {n for n, _ in need} == {'vg_actnorm_bwd', 'vg_actnorm_bwd_stats', 'vg_actnorm_bwd_apply', 'vg_actnorm_bwd_apply2', 'vg_concat_bwd',
                                    'vg_stem_short_fwd', 'vg_stem_short_bwd', 'vg_tanh_bwd'}
    # what no older walk records: all but one regime (they carry N)
    older = set(CR.needed_calls()) | set(CR.ragged_needed_calls())
    fresh = [c for c in need if c not in older]
    assert len(fresh) == 178 and all(c in cov for c in fresh)
    count = lambda name: sum(1 for n, _ in fresh if n == name)
    assert [count(n) for n in ('vg_actnorm_bwd', 'vg_actnorm_bwd_stats', 'vg_actnorm_bwd_apply', 'vg_actnorm_bwd_apply2', 'vg_concat_bwd',
                               'vg_stem_short_fwd', 'vg_stem_short_bwd', 'vg_tanh_bwd')] == [50, 44, 25, 25, 20, 5, 5, 4]
    fin = CR.batch3_needed_fin()
    assert len(fin) >= 30 and not [k for k in fin if ('fin',) + k not in cov]           # no tail dropped: every one is a batch-3 call
    walks = LR.all_batch3_walks()
    cap = LR.macs_cap()
    for cid, c in cases.items():
        assert c['config'] in walks, cid
        if c['kind'] == 'fin':
            r, rec = c['recipe'], c.get('recorded', c['recipe'])
            assert any(x is rec for _, _, _, x in walks[c['config']][0]) and LR.recipe_variant(r) == c['variant'], cid
            assert CR.fin_shape(r) == c['covers'][0][2] and r['src']['N'] in (3, 6) and c['macs'] <= cap, cid
            assert r['fin']['count'] == float(math.prod(LR.out_grid(r))), cid
        elif c['kind'] in ('anb', 'apply2'):
            r = dict(c['regime'] if c['kind'] == 'anb' else c['regime'][0][1])
            assert r['N'] in LR.BATCH3_N, cid
        elif c['kind'] == 'decoder':
            assert c['block']['N'] == 6, cid
        elif c['kind'] in ('stem_short_fwd', 'stem_short_bwd'):
            assert dict(c['regime'])['N'] in (3, 6), cid
    kinds = {c['kind'] for c in cases.values()}
    assert kinds == {'anb', 'apply2', 'decoder', 'fin', 'stem_short_fwd', 'stem_short_bwd', 'tanh_bwd'}, kinds
    # the regimes the step depends on, at batch 3: backward_both's 3B launch (a 2B-sample and a B-sample gradient aliased in one)
    anb = [dict(c['regime']) for c in cases.values() if c['kind'] == 'anb']
    assert any(r['N'] == 9 and r['alias_n0'] > 0 and 0 < r['pgrad_n'] < r['N'] for r in anb)
    assert all((r['alias_n0'], r['alias_shift'], r['pgrad_n']) == (6, 3, 6) for r in anb if r['N'] == 9)
    assert any(r['has_mult'] and r['act'] == 2 for r in anb) and any(r['has_x1'] and r['x0_shift'] for r in anb)
    assert any(r['accumulate'] for r in anb) and any(r['C'] == 1 and r['dx_f32'] for r in anb)
    assert {3, 6, 9} == {r['N'] for r in anb}


def test_decoder_blocks_of_the_batch3_configs_match_the_walks():
    """dec0 and dec1 on the fused split kernel, dec2 and dec3 on the fall-back with vg_concat_bwd, at every batch-3 config, 6 samples."""
    cases = CR.batch3_call_cases()
    for cfg in LR.BATCH3_CONFIGS:
        walk = sorted(tuple(v for k, v in r if k in ('N', 'D', 'H', 'W', 'Cu', 'Cs')) for n, r in LR.all_batch3_walks()[cfg][1] if n == 'vg_concat_bwd')
        blocks = CR.decoder_blocks(cfg, LR.BATCH3_CONFIGS)
        assert walk == sorted((b['N'], *b['dims'], b['c_low'], b['c_skip']) for b in blocks), cfg
        assert [(b['block'], b['served'], b['N']) for b in blocks] == [('dec0', True, 6), ('dec1', True, 6), ('dec2', False, 6), ('dec3', False, 6)]
        for b in blocks:
            assert cases['decoder %s %s' % (b['block'], cfg)]['block'] == b


def test_the_existing_case_lists_are_unchanged():
    """Nothing of this moved what tests/test_gpu_layers.py, test_gpu_infer_layers.py, test_gpu_calls.py and test_gpu_ragged.py run."""
    assert len(LR.representatives()) == len({(k, v) for recs in LR.all_records().values() for k, _, v, _ in recs}) == 154
    assert len(LR.inference_representatives()) == 44 and len(CR.call_cases()) == 137 and len(CR.inference_fin_cases()) == 8
    assert len(LR.ragged_representatives()) == 133 and len(LR.ragged_only_variants()) == 50
    assert all(r['config'] in LR.CONFIGS for r in LR.representatives().values())
    assert all(r['config'] in LR.RAGGED_CONFIGS or r['config'] in LR.RAGGED_INFER_CONFIGS for r in LR.ragged_representatives().values())
    assert all(c['config'] in LR.NEEDED for c in CR.call_cases().values())
    assert all(c['config'] in LR.RAGGED_CONFIGS or c['config'] in LR.RAGGED_INFER_CONFIGS for c in CR.ragged_call_cases().values())
    for other in (CR.call_cases(), CR.ragged_call_cases()):             # ids carry N and the grid (decoder blocks: the config) -- except the tails'
        shared = set(other) & set(CR.batch3_call_cases())
        assert all(other[cid]['kind'] == 'fin' and CR.batch3_call_cases()[cid].get('recorded', CR.batch3_call_cases()[cid]['recipe']) is not other[cid]['recipe']
                   for cid in shared)
