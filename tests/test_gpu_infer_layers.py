"""GPU parity, one layer at a time, for the kernels of the sliding-window inference forward -- ResUNet.forward(save=False) on 128^3
windows, two per batch: what `bench.py --infer` times, in bf16 and in fp16.

bf16 library (libvangan_hip.so): the six variants that only this forward selects (tests/test_variant_coverage.py pins them by name)
replayed at their recorded shapes against the oracle's convolution with the tolerances of tests/test_gpu_layers.py, their InstanceNorm
finalisation tails against float64 statistics of the stored output, and the K-split exchange of the `|ks4` variant bitwise over 200
launches on two streams.

fp16 library (libvangan_hip_h.so, the same sources with -DVG_FP16: f16 MFMA opcodes, IEEE-half bf2f / f2bf): EVERY forward variant of the
two inference walks replayed inside ops.Fp16() on torch.float16 tensors, the reference rounding with .half() where it rounds to bf16 for
the other library -- output, residual / tanh / f32-output branches and the `sums` statistics.  The bounds are the bf16 ones scaled by
2^-3 (layer_recipes.FWD_TOL; derived from the significand widths, held by the reference alone in
tests/test_variant_coverage.py::test_fp16_bound_holds_for_the_reference_alone).  Then what those replays rest on, bitwise: the storage
conversions of both libraries over special values, vg_pack_weights of the fp16 library, and the stem shortcut's scale / shift with its
weight rounded to fp16.

Not covered here: the ResNet and attention-gated generators' inference walks, fp16 subnormal OPERANDS through the matrix pipe (operand
magnitudes are O(1), as everywhere in layer_recipes), the whole-network fp16 bounds, and any timing.

Measured on an MI355X (max |err| / max |ref| of the stored output; rel-L2 of the statistics and of an fp32 output):
  bf16 library, the six inference-only variants        output 2.0e-3 .. 3.3e-3   statistics 1.8e-7 .. 8.2e-7
  bf16 library, their eight finalisation tails          scale / shift / mean / rstd 4.9e-8 .. 3.0e-7 (bound 1e-4)
  fp16 library, 24 variants with a 16-bit output        output 2.3e-4 .. 4.1e-4 (half an fp16 ulp at max |ref|: 4.9e-4)   statistics 6.2e-8 .. 1.0e-6
  fp16 library, pw_cto1 (tanh into the fp32 volume)     5.2e-8 (bound 1e-4)
  fp16 library, stem shortcut                           scale 3.5e-8, shift 3.8e-8 (bound 1e-5)
  conversions, weight packing                           bitwise"""
import math

import pytest
import torch

import call_recipes as CR
import layer_recipes as LR

pytestmark = pytest.mark.gpu

_REPS = LR.inference_representatives()
_NEW = LR.inference_only_variants()
_ALL = sorted(LR.inference_needed_variants(), key=lambda kv: _REPS[kv]['macs'])
_FIN = CR.inference_fin_cases()


def _dev():
    return torch.device('cuda:0')


def _id(kv):
    r = _REPS[kv]
    return '%s [%s %s N%d %s]' % (kv[1], r['config'], r['layer'], r['recipe']['src']['N'], 'x'.join(str(n) for n in r['recipe']['src']['dims']))


def _report(name, err):
    print('%-100s %s' % (name, '  '.join('%s %.2e' % kv for kv in sorted(err.items()))))


# ----------------------------------------------------------------------------------------------------------------------
# bf16 library: the variants only the inference forward selects
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kv', _NEW, ids=[_id(kv) for kv in _NEW])
def test_inference_only_variant_matches_oracle(kv):
    err = LR.run_recipe(_REPS[kv]['recipe'], kv[1], _dev(), arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))
    _report('bf16 ' + _id(kv), err)


_KSPLIT = [kv for kv in _NEW if kv[1].startswith('conv<') and kv[1].rsplit('|ks', 1)[-1] not in ('0', '1')]


def test_inference_ksplit_case_exists():
    assert [v for _, v in _KSPLIT] == ['conv<bf16,32,1,n0,wl0,dma0,mc0,c10>|walk0|ch1|ks4']


@pytest.mark.parametrize('kv', _KSPLIT, ids=[_id(kv) for kv in _KSPLIT])
def test_inference_ksplit_exchange_is_bitwise_stable_under_load(kv):
    """enc4.cb1 / enc4.cb2 / bridge.cb1 / bridge.cb2 of the two-window batch: four K slices exchange partial tiles through the per-stream
    scratch (tests/test_gpu_layers.py has the argument).  200 launches on two streams must reproduce the first bit for bit."""
    LR.stress_recipe(_REPS[kv]['recipe'], kv[1], _dev(), launches=200, arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))


@pytest.mark.parametrize('cid', sorted(_FIN))
def test_inference_finalisation_tail_matches_float64(cid):
    c = _FIN[cid]
    _report(cid, dict(fin=CR.run_fin(c['recipe'], c['variant'], _dev(), arena=LR.guarded_for(c['recipe'], _dev()))))


# ----------------------------------------------------------------------------------------------------------------------
# fp16 library: every forward variant of the inference walks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kv', _ALL, ids=[_id(kv) for kv in _ALL])
def test_fp16_build_layer_variant_matches_oracle(kv):
    """Identical fp16-rounded operands into kernel and reference: what differs is the fp32 accumulation order and the one rounding of the
    stored output, so the bounds are run_recipe's bf16 ones times 2^-3: close(rel=1.5e-3, floor=2.5e-4 max|ref|), statistics rel-L2 <
    2.5e-3, f32 output rel-L2 < 1e-4."""
    from van_gan_amd import ops
    with ops.Fp16():
        assert ops.lib.vg_storage16() == 1
        err = LR.run_recipe(_REPS[kv]['recipe'], kv[1], _dev(), storage=torch.float16, arena=LR.guarded_for(_REPS[kv]['recipe'], _dev()))
    _report('fp16 ' + _id(kv), err)


def test_fp16_cases_cover_the_branches():
    rs = [_REPS[kv]['recipe'] for kv in _ALL]
    assert len(_ALL) >= 25 and all(r['kind'] == 'fwd' for r in rs)
    assert any(r['res'] and not r.get('res_c1') for r in rs) and any(r.get('res_c1') for r in rs)       # residual: stored tensor, fp32 volume
    assert any(r['tanh'] and r['out_f32'] for r in rs) and any(r['sums'] for r in rs)
    assert any(r['src']['shift0'] and r['src']['c1'] for r in rs) and any(r['src']['f32'] for r in rs)  # virtual upsample + concat; fp32 source
    fams = {v.split('<')[0] for _, v in _ALL}
    assert fams == {'conv', 'conv32', 'conv_thin', 'conv_thin2', 'c1m_fwd', 'pw_gemm', 'pw_cto1'}, fams


# ----------------------------------------------------------------------------------------------------------------------
# the storage conversions, both libraries, bitwise
# ----------------------------------------------------------------------------------------------------------------------
def _special_values():
    """fp32 bit patterns where a conversion to 16 bits goes wrong first."""
    f = lambda *v: torch.tensor(v, dtype=torch.float32)
    bits = lambda *v: torch.tensor(v, dtype=torch.int32).view(torch.float32)
    inf, nan = float('inf'), float('nan')
    parts = [
        f(0.0, -0.0, inf, -inf, nan, -nan),
        bits(0x7FC00001, 0x7F800001, 0x7FFFFFFF),                 # quiet / signalling NaN payloads
        # exact ties of bf16 (low 16 bits = 0x8000; even and odd kept bit) and their neighbours
        bits(0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001),
        # exact ties of fp16 (low 13 bits = 0x1000) and their neighbours
        bits(0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001, 0x3F802FFF, 0x3F803001),
        # the fp16 overflow boundary: 65504 is the largest finite half, 65520 the tie that rounds to infinity
        f(65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, -65504.0, -65519.996, -65520.0, 1e5),
        # the largest bf16 (0x7F7F0000), the fp32 values above it that still round to it / to infinity, the largest fp32
        bits(0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF),
        # the fp16 subnormal range: 2^-24 k, half of the smallest subnormal (a tie to zero) and its neighbours, the smallest normal
        f(*[k * 2.0 ** -24 for k in (1, 2, 3, 1023, 1024, 1025)], 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -25 * (1 - 2.0 ** -20),
          1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -26, -2.0 ** -25, -1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12)),
        torch.logspace(math.log10(2.0 ** -27), math.log10(2.0 ** -13), 4096),
        -torch.logspace(math.log10(2.0 ** -27), math.log10(2.0 ** -13), 4096),
        # fp32 subnormals (bf16 has fp32's exponent range: they are bf16 subnormals)
        bits(0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00400000),
    ]
    return torch.cat(parts)


def _same_bits16(got, want, what):
    """Bitwise on everything that is not NaN; NaN-ness where either is NaN."""
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    assert torch.equal(gn, wn), '%s: NaN-ness differs at %d elements' % (what, int((gn != wn).sum()))
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    bad = (gi != wi) & ~wn
    assert not bool(bad.any()), '%s: %d elements differ, first at %d: got 0x%04x want 0x%04x' % (
        what, int(bad.sum()), int(bad.nonzero()[0]), int(gi[bad][0]) & 0xFFFF, int(wi[bad][0]) & 0xFFFF)


@pytest.mark.parametrize('storage', [torch.bfloat16, torch.float16], ids=['bf16 library', 'fp16 library'])
def test_storage_conversions_are_bitwise_rne(storage):
    """vg_f32_to_bf16 / vg_bf16_to_f32 (f2bf / bf2f of the build, which every epilogue and every staging load goes through) against
    torch's .to(torch.bfloat16) / .half() and .float(): round to nearest even incl. ties, overflow to infinity at the format's boundary,
    subnormals, signed zeros -- about 2^20 values, a length that is no multiple of 8 (no vector tail may be dropped or overrun)."""
    from van_gan_amd import ops
    from van_gan_amd._lib import check
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, ((1 << 20) - 5000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    x = torch.cat([_special_values(), rnd, torch.randn(3, generator=g)])
    n = x.numel()
    assert n % 8 != 0 and abs(n - (1 << 20)) < (1 << 14)
    import guarded
    ga = guarded.GuardedArena(16 * (n + (1 << 17)) + 4 * guarded.slot_cost(0), dev)     # inputs sealed; outputs keep their 8 guard elements too
    xd = ga.put(x, name='x')
    y = ga.out((n + 8,), storage, 1.0, name='y')                              # 8 guard elements behind the end
    want = x.to(storage)                                                      # CPU: IEEE round to nearest even
    patterns = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(storage)        # every 16-bit pattern
    back_in = ga.put(torch.cat([patterns, want]), name='back_in')
    back = ga.out((back_in.numel() + 8,), torch.float32, 7.0, name='back')
    ctx = ops.Fp16() if storage == torch.float16 else None
    if ctx is not None:
        ctx.__enter__()
    try:
        assert ops.lib.vg_storage16() == int(storage == torch.float16)
        check(ops.lib.vg_f32_to_bf16(xd.data_ptr(), y.data_ptr(), n, ops.stream()), 'vg_f32_to_bf16')
        check(ops.lib.vg_bf16_to_f32(back_in.data_ptr(), back.data_ptr(), back_in.numel(), ops.stream()), 'vg_bf16_to_f32')
        torch.cuda.synchronize()
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    _same_bits16(y[:n].cpu(), want, 'f32 -> 16 bit')
    assert bool((y[n:] == 1.0).all()) and bool((back[back_in.numel():] == 7.0).all()), 'written past the end'
    bw, bg = back_in.cpu().float(), back[:back_in.numel()].cpu()
    gn, wn = torch.isnan(bg), torch.isnan(bw)
    assert torch.equal(gn, wn)
    assert torch.equal(bg.view(torch.int32)[~wn], bw.view(torch.int32)[~wn]), '16 bit -> f32 is exact'
    ga.verify()


# ----------------------------------------------------------------------------------------------------------------------
# vg_pack_weights of the fp16 library
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,cin,cout,stride,pad', [(3, 32, 64, 2, 'reflect'), (1, 48, 16, 1, 'same')], ids=['3^3 32->64 stride 2', '1^3 48->16'])
def test_fp16_build_packs_rne_half_weights(k, cin, cout, stride, pad):
    """Every element of every packed operand of a layer (forward, and each output-parity class of the data gradient) is the RNE fp16
    rounding of its weight; padding stays zero.  The packing is a permutation (plus zero padding) that both builds share, and the bf16
    library packs a bf16-exact tensor without rounding: w = hi + mid + lo with three bf16-exact terms (8 + 8 + 8 significand bits) is
    packed term by term on the bf16 library and summed in fp32 -- the exact fp32 weight at every packed position -- and .half() of that
    must be what the fp16 library wrote, bit for bit."""
    from van_gan_amd import ops
    dev = _dev()
    ctor = dict(k=k, cin=cin, cout=cout, stride=stride, pad=pad, bias=True, in_dims=(8, 16, 16), need_dgrad=True)
    st0, _ = LR.make_layer_from(ctor, 'cpu', seed=4)
    w = st0.param('c.w').clone()
    w.view(-1)[:6] = torch.tensor([65504.0, 2.0 ** -24, 3 * 2.0 ** -25, -(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11, 0.0])     # boundary, subnormal, ties
    hi = LR.bf(w)
    mid = LR.bf(w - hi)
    lo = LR.bf(w - hi - mid)
    assert torch.equal(hi + mid + lo, w) and torch.equal((w - hi - mid) - lo, torch.zeros_like(w))

    def packed(part, dtype):
        st, lay = LR.make_layer_from(ctor, dev, seed=4, dtype=dtype)
        st.param('c.w').copy_(part)
        items = lay.pack_items()
        for it in items:
            it[2].fill_(7.0)                                       # the pack must write every element, padding included
        lay.pack()
        torch.cuda.synchronize()
        return [it[2].clone() for it in items]

    exact = None
    for part in (hi, mid, lo):
        p = [t.float() for t in packed(part, torch.bfloat16)]
        exact = p if exact is None else [a + b for a, b in zip(exact, p)]
    with ops.Fp16():
        got = packed(w, torch.float16)
    assert len(got) == len(exact) >= 2
    n = 0
    for a, e in zip(got, exact):
        assert a.dtype == torch.float16 and a.shape == e.shape
        _same_bits16(a.cpu().view(-1), e.cpu().half().view(-1), 'packed operand %d' % n)
        n += int((e != 0).sum())
    assert n >= 2 * (w.numel() - 1) - 8                             # forward + the data-gradient classes: every weight twice


# ----------------------------------------------------------------------------------------------------------------------
# vg_stem_short_fwd of the fp16 library
# ----------------------------------------------------------------------------------------------------------------------
def test_fp16_build_stem_shortcut_scale_and_shift():
    """The regime the inference walk records (two 128^3 windows, 16 channels, round16 = 1): scale / shift of IN(w x + b) from the volume's
    mean and variance, the 1x1x1 weight rounded to the build's 16-bit format -- fp16 here.  The float64 restatement of
    tests/test_gpu_ops.py::test_stem_shortcut_as_an_affine_function_of_the_volume with .half() where it rounds to bf16, its bound 1e-5
    (nothing else is rounded to 16 bits: the bound does not scale).  The weights are chosen so that fp16 and bf16 rounding differ by far
    more than the bound."""
    from van_gan_amd import ops
    dev = _dev()
    reg = [dict(r) for n, r in LR.all_inference_walks()['infer 128^3 N2'][1] if n == 'vg_stem_short_fwd']
    assert len(reg) == 1 and reg[0]['round16'] == 1
    N, S, C_ = reg[0]['N'], reg[0]['S'], reg[0]['C']
    assert (N, S, C_) == (2, 128 ** 3, 16) and reg[0]['G'] == int(ops.lib.vg_stem_short_fwd_workgroups(N, S))
    g = torch.Generator(device=dev).manual_seed(21)
    x = torch.rand(N, S, 1, generator=g, device=dev) * 2 - 1
    x[N - 1] = x[N - 1] * 0.3 + 0.5                                  # samples with different mean / variance
    w = torch.randn(C_, generator=g, device=dev) * 0.4
    w[3] = 0.01
    gam, bet = torch.rand(C_, generator=g, device=dev) + 0.5, torch.randn(C_, generator=g, device=dev) * 0.1
    import guarded
    ga = guarded.GuardedArena(4 * N * S + (1 << 20) + 6 * guarded.slot_cost(0), dev)
    x, w, gam, bet = ga.put(x, name='x'), ga.put(w, name='w'), ga.put(gam, name='gamma'), ga.put(bet, name='beta')
    sc, sh = ga.out((N, C_), torch.float32, None, name='scale'), ga.out((N, C_), torch.float32, None, name='shift')
    with ops.Fp16():
        ar = ops.Arena(64 << 20, dev)
        ops.stem_short_fwd(ar, x, N, C_, w, gam, bet, sc, sh, round16=True)
        torch.cuda.synchronize()
    xd = x.double().view(N, S)
    mu, var = xd.mean(1), xd.var(1, unbiased=False)

    def restate(wq):
        rs = (wq[None] ** 2 * var[:, None] + ops.IN_EPS).rsqrt()
        s = gam.double()[None] * wq[None] * rs
        return s, bet.double()[None] - s * mu[:, None]
    ref_sc, ref_sh = restate(w.half().double())
    err = dict(scale=LR.rel_l2(sc, ref_sc), shift=LR.rel_l2(sh, ref_sh))
    _report('fp16 stem_short_fwd N%d S%d' % (N, S), err)
    assert err['scale'] <= 1e-5 and err['shift'] <= 1e-5, err
    other = restate(w.bfloat16().double())                            # the check tells the two roundings apart
    assert LR.rel_l2(other[0], ref_sc) > 1e-4
    ga.verify()
