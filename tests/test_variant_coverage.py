"""CPU: every kernel variant that BASELINE configs 2, 3 and 4 run has a parity case on the GPU (tests/test_gpu_layers.py), and so has
every variant of the sliding-window inference forward, on the bf16 and on the fp16 library (tests/test_gpu_infer_layers.py).

The kernels pick a template instantiation per launch (channel panel, voxel tile, weights in LDS or L2, fused / class-parallel
output-parity classes, single-channel staging, the 32x32x16 flavour, weight-gradient slab shapes ...), and the choice depends
on the problem size -- so a parity suite made of small hand-picked shapes can be green while the kernels the benchmark
times are never compared with the oracle.  Here the real schedules are walked in dry-run mode (tests/layer_recipes.py) and
the variant of every convolution launch is collected through vg_conv3d_variant / vg_conv3d_wgrad_variant."""
import pytest
import torch

import call_recipes as CR
import layer_recipes as LR


def test_every_variant_of_the_baseline_configs_has_a_gpu_parity_case():
    reps = LR.representatives()
    needed = LR.needed_variants()
    assert len(needed) >= 60                       # sanity: the walk saw the whole step
    missing = [kv for kv in needed if kv not in reps]
    assert not missing, missing
    # the GPU test is parametrised over exactly these representatives; each is a call of a real layer at its true shape
    for kv in needed:
        r = reps[kv]
        assert r['config'] in LR.CONFIGS and r['recipe']['kind'] == kv[0]
    # kinds of kernels that must be present: both MFMA flavours, fused and class-parallel strided data gradients, the
    # single-channel staging variant, the pointwise kernels, the three weight-gradient slab families (the DMA one with the materialised operand, d0, and copying the stored tensors, d1), the K-split deep-level launches (ks), the thin-channel specialist
    # (both staging modes) and the shortcut-convolution kernels (forward with geometry, dense and strided accumulating data gradient, the DMA weight gradient
    # of the 1x1x1 layers in every instantiation, with the virtual upsample + concat and with stride 2)
    names = ' '.join(v for _, v in needed)
    for frag in ('conv<bf16,16,8', 'conv<bf16,32,4', 'conv32<128', 'conv32<64', 'mc1', 'mc2', 'cp1', 'c11', 'pw_cto1', 'pw_1toc',
                 'c1m_fwd<f32,3,1,1,n0>', 'c1m_wgrad<f32,3,1,1,n0>', 'c1m_fwd<f32,4,2,4,n1>', 'c1m_wgrad<f32,4,2,4,n1>', 'wgrad<bf16,24,1', 'wgrad<bf16,7,4', 'walk1', 'ch1', 'part1', 'n1',
                 'wgrad_dma<4,1,d0>', 'wgrad_thin<m1>|ch0', 'wgrad_thin<m1>|ch1', 'wgrad_dma<4,2,d0>', 'wgrad_dma<4,2,d1>', 'wgrad_dma<8,2,d0>', 'wgrad_dma<8,4,d0>', '|s2|', '|nb3|', '|ks4', '|ks2',
                 'conv_thin<m0', 'conv_thin<m1', 'pw_gemm<2,1,g1,a0>', 'pw_gemm<1,3,g0,a1>', 'pw_gemm<1,1,g1,a1>',
                 'wgrad_pw_dma<3,1>', 'wgrad_pw_dma<6,2>', 'wgrad_pw_dma<4,4>', 'wgrad_pw_dma<6,4>', '|s1|u1|', '|s2|u0|',
                 # the LDS-DMA forward / data-gradient family: both panel widths, 4^3 and 3^3 stage bodies, K split, class-parallel strided
                 # data gradients, launches with more units than CUs
                 # the two-panel instance of the thin-channel specialist (32-channel layers at 64^3), forward and data gradient
                 'conv_thin2<m1', 'conv_thin2<m0',
                 # ... and its panel loop (dec0.cb1's 16 -> 48 data gradient with the IN-backward statistics: three panels over one staged halo)
                 'bs2,pl>',
                 'conv_dma<128,256>', 'conv_dma<64,256>', '|gt8|', '|gt9|', 'ks1|cls0', 'ks0|cls1', 'cls1|walk1'):
        assert frag in names, frag


# what only the sliding-window inference forward (two 128^3 windows per batch) selects: no train step of BASELINE configs 1-4 launches these
INFERENCE_ONLY = {
    'conv_thin2<m1,b1,r1,s1>|walk1|ch1',                            # enc1.cb2, dec1.cb2
    'conv_thin2<m1,b1,r0,s1>|walk1|ch1',                            # dec1.cb1
    'conv<bf16,64,2,n0,wl0,dma0,mc0,c10>|walk1|ch0|ks1',            # enc2.cb1
    'conv32<128,1,n0,cp0>|walk0|ch1',                               # enc3.cb1, enc3.cb2, dec3.short, dec3.cb1, dec3.cb2
    'conv<bf16,32,1,n0,wl1,dma0,mc0,c10>|walk0|ch1|ks1',            # enc4.short
    'conv<bf16,32,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks4',            # enc4.cb1, enc4.cb2, bridge.cb1, bridge.cb2: the K-split exchange
}


def test_every_variant_of_the_inference_forward_has_a_gpu_parity_case():
    """The published inference line (bench.py --infer) runs ResUNet.forward(save=False) on 128^3 windows, two per batch (one in the tail
    batch of an odd window count).  Its launches are walked like the train steps'; every variant has a representative that
    tests/test_gpu_infer_layers.py replays (the inference-only ones on the bf16 library, all of them on the fp16 library), and the set of
    inference-only variants is pinned BY NAME: a dispatch change that moves the inference path onto other kernels fails here."""
    walks = LR.all_inference_walks()
    for cfg in LR.INFER_NEEDED:
        recs = walks[cfg][0]
        assert [k for k, _, _, _ in recs] == ['fwd'] * 29, cfg              # 29 convolution launches, no other kind
        assert [n for n, _ in walks[cfg][1]] == ['vg_stem_short_fwd']       # and the stem shortcut as an affine function of the volume
    reps, needed = LR.inference_representatives(), LR.inference_needed_variants()
    missing = [kv for kv in needed if kv not in reps]
    assert not missing, missing
    for kv in needed:
        r = reps[kv]
        assert r['recipe']['kind'] == 'fwd' and (r['config'] in LR.INFER_CONFIGS or r['config'] in LR.CONFIGS)
        assert r['macs'] <= max(x['macs'] for x in LR.representatives().values())          # no case heavier than test_gpu_layers.py's heaviest
        assert LR.recipe_variant(r['recipe']) == kv[1], kv                  # a shrunk representative still selects the identical variant
    new = {v for _, v in LR.inference_only_variants()}
    assert new == INFERENCE_ONLY, (sorted(new - INFERENCE_ONLY), sorted(INFERENCE_ONLY - new))
    assert not {v for k, _, v, _ in walks['infer 128^3 N1'][0]} & INFERENCE_ONLY          # all of them come from the two-window batch


@pytest.mark.parametrize('cfg', LR.INFER_NEEDED)
def test_fp16_network_selects_the_same_variants(cfg):
    """The dispatch is host logic shared by libvangan_hip.so and libvangan_hip_h.so: a torch.float16 network walks the same variant strings."""
    dims, N = LR.INFER_CONFIGS[cfg]
    h = LR.walk_inference(dims, N, torch.float16)
    assert [(k, n, v) for k, n, v, _ in h[0]] == [(k, n, v) for k, n, v, _ in LR.all_inference_walks()[cfg][0]]
    assert h[1] == LR.all_inference_walks()[cfg][1]


def test_every_finalisation_tail_of_the_inference_forward_has_a_gpu_case():
    """The out_jobs of ResUNet._block_fwd: each (forward variant, tail job shape) of the inference walks is already one of the train steps'
    (call_recipes.needed_fin, replayed by tests/test_gpu_calls.py) or has a run_fin case in tests/test_gpu_infer_layers.py."""
    have = set(CR.needed_fin())
    cov = {c['covers'][0][1:] for c in CR.inference_fin_cases().values()}
    need = CR.inference_needed_fin()
    assert len(need) >= 20
    missing = [k for k in need if k not in have and k not in cov]
    assert not missing, missing
    assert {v for v, _ in cov} == INFERENCE_ONLY and not cov & have       # exactly the inference-only variants carry new tails
    for c in CR.inference_fin_cases().values():
        r = c['recipe']
        assert LR.recipe_variant(r) == c['variant'] and CR.fin_shape(r) == c['covers'][0][2]
        assert r['fin']['count'] * r['layer']['stride'] ** 3 == float(torch.tensor(r['src']['dims']).prod())


def test_fp16_bound_holds_for_the_reference_alone():
    """The fp16 bounds of layer_recipes.FWD_TOL are the bf16 ones scaled by 2^-3 (11 significand bits against 8), not measured on the
    kernels.  Here the reference itself is held to them: a float32 convolution of the fp16-rounded operands followed by .half() -- what a
    correct kernel computes, up to accumulation order -- against the float64 restatement, on the 32^3 walk's enc2.cb1 call (32 -> 64
    channels, stride 2, on-read InstanceNorm + ReLU, 864-term sums).  No element may fall outside."""
    from oracle import vangan_oracle as O
    recipe = next(r for _, n, _, r in LR.all_inference_walks()['infer 32^3 N2'][0] if n == 'enc2.cb1.conv')
    L, sr, st16 = recipe['layer'], recipe['src'], torch.float16
    g = torch.Generator().manual_seed(1)
    st, _ = LR.make_layer_from(L, 'cpu', dtype=st16)
    _, host = LR.make_operand(sr, L['pad'], 'cpu', g, st16)
    tol = LR.FWD_TOL[st16]
    assert tol == dict(rel=LR.FWD_TOL[torch.bfloat16]['rel'] / 8, floor=LR.FWD_TOL[torch.bfloat16]['floor'] / 8,
                       sums=LR.FWD_TOL[torch.bfloat16]['sums'] / 8, f32=1e-4)
    ys = {}
    for dt in (torch.float64, torch.float32):
        ap = LR.ref_operand(sr, host, L['pad'], dt, st16)
        assert torch.equal(ap, ap.half().to(dt))                          # operands are fp16 values in both
        w = LR.bf(st.param('c.w').to(dt), st16)
        ys[dt] = O.to_ndhwc(O.conv3d(ap, w, st.param('c.b').to(dt), L['stride'], 'valid'))
    got, ref = ys[torch.float32].half(), ys[torch.float64]
    assert got.shape == (sr['N'], 8, 8, 8, 64) and float(ref.abs().max()) > 1.0
    LR.close_bf16(got, ref, 'float32 reference + .half()', rel=tol['rel'], floor=tol['floor'])
    sums = lambda y: torch.stack([y.sum(dim=(1, 2, 3)), (y ** 2).sum(dim=(1, 2, 3))], dim=-1)
    assert LR.rel_l2(sums(got.float()), sums(LR.bf(ref, st16))) < tol['sums']
    # and the bound is not vacuous: the same result rounded to bf16 instead is far outside it
    with pytest.raises(AssertionError):
        LR.close_bf16(ys[torch.float32].bfloat16(), ref, 'bf16 rounding', rel=tol['rel'], floor=tol['floor'])


def test_resnet_generator_walk():
    """the kernel variants the ResNet generator launches at the 128^3 patch are all exercised by its teacher-forced GPU
    tests (tests/test_gpu_resnet.py runs the whole network, forward and backward, at 32^3 batch 2, 64^3 and 128^3 -- the walk below
    is what those runs launch), and the families one expects are there: the W-packed 7^3 stem, the seven 49-tap chunks of the head,
    class-parallel strided data gradients on odd grids, the LDS-DMA data gradients and weight gradients of the 256-channel trunk."""
    sizes = {'32^3 B2': ((32, 32, 32), 2), '64^3 B1': ((64, 64, 64), 1), '128^3 B1': ((128, 128, 128), 1)}
    recs = {k: LR.enumerate_resnet(*v) for k, v in sizes.items()}
    var = {k: {(kind, v) for kind, _, v in r} for k, r in recs.items()}
    assert len(recs['128^3 B1']) == 77                      # 26 convolutions: 32 forward launches (head: 7), 32 + 13 backward
    only_128 = var['128^3 B1'] - var['64^3 B1'] - var['32^3 B2']
    assert len(only_128) >= 4, sorted(only_128)             # why the 128^3 GPU test exists (13 variants no smaller grid selects)
    names = ' '.join(v for k in var for _, v in var[k])
    for frag in ('c11', 'conv32<128', 'conv32<64', 'cp1', 'mc1', 'conv_dma<128,256>', 'wgrad_dma<8,2,d0>', 'wgrad_dma<8,4,d0>', 'wgrad<bf16,7,4'):
        assert frag in names, frag
    heads = [n for kind, n, _ in recs['128^3 B1'] if kind == 'fwd' and n == 'out']
    assert len(heads) == 7


def test_walk_is_complete():
    """One generator application is 29 forward + 29 weight-gradient + 28 data-gradient calls (the stem's shortcut is no convolution
    launch in either direction: forward an affine function of the volume added in stem.cb's epilogue, vg_stem_short_fwd / res_c1,
    backward a closed form in two moments, vg_stem_short_bwd; stem.conv1 has no data gradient), one discriminator 5 + 5 + 2 x 5 (the
    second sweep stops at the input volume)."""
    recs = LR.all_records()['32^3 B1']
    kinds = [k for k, _, _, _ in recs]
    names = {n for _, n, _, _ in recs}
    assert kinds.count('fwd') == 34 and kinds.count('wgrad') == 34
    assert {'stem.conv1', 'dec0.cb1.conv', 'bridge.cb2.conv', 'out', 'conv0', 'down2'} <= names


@pytest.mark.parametrize('cfg', LR.NEEDED)
def test_variant_names_are_stable_within_a_config(cfg):
    """The same call selects the same variant when asked twice (the dispatch has no hidden state)."""
    dims, B = LR.CONFIGS[cfg]
    a = LR.enumerate_config(dims, B)
    assert [(k, n, v) for k, n, v, _ in a] == [(k, n, v) for k, n, v, _ in LR.all_records()[cfg]]
