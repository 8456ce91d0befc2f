"""CPU: every non-convolution call that BASELINE configs 2, 3 and 4 make -- InstanceNorm backward (statistics, apply, two-job apply),
the decoder blocks' concat backward, the stem shortcut, tanh backward -- and every forward launch that carries the InstanceNorm
finalisation tail has a GPU parity case at its true shape (tests/test_gpu_calls.py).  The regimes come from the same dry-run walk as
the convolution variants (tests/call_recipes.py); this file proves the case list covers them."""
import layer_recipes as LR
import call_recipes as CR


def _covered():
    return {c for case in CR.call_cases().values() for c in case['covers']}


def test_every_recorded_call_regime_has_a_gpu_case():
    need = CR.needed_calls()
    cov = _covered()
    missing = [c for c in need if c not in cov]
    assert not missing, missing[:5]
    names = {n for n, _ in need}
    assert names == {'vg_actnorm_bwd', 'vg_actnorm_bwd_stats', 'vg_actnorm_bwd_apply', 'vg_actnorm_bwd_apply2', 'vg_concat_bwd',
                     'vg_stem_short_fwd', 'vg_stem_short_bwd', 'vg_tanh_bwd'}, names
    # the ConvLayer recipes are not changed by the new recording
    for cfg in LR.NEEDED:
        recs = CR.all_walks()[cfg][0]
        assert [(k, n, v) for k, n, v, _ in recs] == [(k, n, v) for k, n, v, _ in LR.all_records()[cfg]]


def test_regimes_the_step_depends_on_are_recorded():
    anb = [dict(r) for n, r in CR.needed_calls() if n in CR.ANB_ENTRIES]
    jobs = [dict(j) for n, r in CR.needed_calls() if n == 'vg_actnorm_bwd_apply2' for _, j in r]
    assert any(r['alias_n0'] > 0 and r['alias_shift'] > 0 and 0 < r['pgrad_n'] < r['N'] for r in anb)      # PatchGAN.backward_both
    assert any(r['has_mult'] and r['act'] == 2 for r in anb)                                             # dropout after LeakyReLU
    assert any(r['has_x1'] and r['x0_shift'] for r in anb)                                                # virtual upsample + concat
    assert any(r['accumulate'] for r in anb) and any(r['C'] == 1 and r['dx_f32'] for r in anb)
    assert {48, 96, 192, 384} <= {r['C'] for r in anb}                   # vpb = 256 / (C / 8) leaves threads idle
    assert jobs and any(j['g_padded'] for j in jobs) and any(not j['g_padded'] for j in jobs)
    assert any(r['g_padded'] and min(r['D'], r['H'], r['W']) == 4 for r in anb)


def test_every_finalisation_tail_shape_has_a_gpu_case():
    need = CR.needed_fin()
    cov = _covered()
    missing = [k for k in need if ('fin',) + k not in cov]
    assert not missing, missing
    shapes = {s for _, s in need}
    assert ((False, False),) in shapes and ((True, False),) in shapes and ((False, False), (False, True)) in shapes
    fams = {v.split('<')[0] for v, _ in need}
    assert {'conv_thin', 'conv', 'c1m_fwd', 'pw_gemm'} <= fams, fams
    assert set(CR.fin_stress_cases()) == {'vg_conv_thin', 'vg_conv', 'vg_c1k3', 'vg_pointwise'}


def test_decoder_fused_launches_are_listed_per_config():
    """The fused decoder launches are not taken in dry-run mode; the explicit list must match the walk's fallback concat backward."""
    for cfg in LR.NEEDED:
        walk = sorted(tuple(v for k, v in r if k in ('N', 'D', 'H', 'W', 'Cu', 'Cs')) for n, r in CR.all_walks()[cfg][1] if n == 'vg_concat_bwd')
        listed = sorted((b['N'], *b['dims'], b['c_low'], b['c_skip']) for b in CR.decoder_blocks(cfg))
        assert walk == listed, (cfg, walk, listed)
        assert [b['block'] for b in CR.decoder_blocks(cfg)] == ['dec0', 'dec1', 'dec2', 'dec3']
        assert all('decoder %s %s' % (b['block'], cfg) in CR.call_cases() for b in CR.decoder_blocks(cfg))
