"""The small kernels behind the Wasserstein head and two helpers, each against a float64 reference of the same operation on the same fp32
(or bf16-valued) inputs: vg_dense_head_fwd / vg_dense_head_bwd / vg_wasserstein_terms (vg_loss.hip), vg_bias_grad and vg_axpby
(vg_elem.hip), and vg_local_exchange (vg_adam.hip), which no test reached.  The whole-step tests reach them at one shape each (n = 64 patch logits: one loop trip, one block); the product runs
n = 512, 2048 and 4096.  Every output buffer carries guard cells behind its last element, which must come back untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 32


def rel_l2(got, ref):
    got, ref = got.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def _rand(g, *shape, lo=0.5, hi=1.5, signed=False):
    """Unit-scale values away from zero; signed=True gives them random signs."""
    t = torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo
    if signed:
        t = t * (torch.randint(0, 2, shape, generator=g, dtype=torch.float64) * 2 - 1)
    return t.float()


def _guarded(vals, fill=None):
    """Device buffer [len + GUARD] whose head holds `vals` (or `fill`) and whose tail holds a sentinel pattern; returns (buffer, head view,
    copy of the tail)."""
    n = vals if isinstance(vals, int) else vals.numel()
    buf = torch.empty(n + GUARD, dtype=torch.float32, device=DEV)
    buf[n:] = torch.arange(GUARD, dtype=torch.float32, device=DEV) * 0.25 - 11.0
    if isinstance(vals, int):
        buf[:n] = fill
    else:
        buf[:n] = vals.reshape(-1).to(DEV)
    return buf, buf[:n], buf[n:].clone()


# ------------------------------------------------------------------------------------------------------------------------------------
# Dense(1) over the flattened, dropout-masked patch logits.
# Bound 1e-5 (rel-L2 against float64): an fp32 sum of n <= 4096 unit-scale terms errs by at most n 2^-24 relative to sum |terms|
# however it is ordered; the forward sums n / 256 terms per lane and then 256 lanes as a tree, (n / 256 + 8) 2^-24 <= 1.5e-6 for terms
# of one sign (x, w and the mask are positive here, so sum |terms| is the sum), the backward sums N <= 4 terms.
# ------------------------------------------------------------------------------------------------------------------------------------
HEAD_N = (1, 64, 255, 256, 257, 512, 2048, 4096)
HEAD_TOL = 1e-5


@pytest.mark.parametrize('N', [1, 2, 4])
@pytest.mark.parametrize('n', HEAD_N)
def test_dense_head_fwd_bwd(n, N):
    from van_gan_amd import ops
    g = torch.Generator().manual_seed(1000 * N + n)
    x, w, b = _rand(g, N, n), _rand(g, n), _rand(g, 1)
    mask = (torch.rand(N, n, generator=g) >= 0.2).float() / 0.8
    gz = _rand(g, N, signed=True)
    dw0, db0 = _rand(g, n, signed=True), _rand(g, 1, signed=True)
    xd, wd, bd, md, gzd = (t.to(DEV) for t in (x, w, b, mask, gz))
    for use_mask, use_b in ((True, True), (False, True), (True, False)):
        m64 = mask.double() if use_mask else torch.ones(N, n, dtype=torch.float64)
        what = 'n %d N %d mask %s b %s' % (n, N, use_mask, use_b)
        # forward
        zbuf, z, ztail = _guarded(N, fill=7.0)
        ops.dense_head_fwd(xd, md if use_mask else None, wd, bd if use_b else None, N, n, z)
        z_ref = (x.double() * m64 * w.double()).sum(1) + (b.double() if use_b else 0.0)
        e = rel_l2(z, z_ref)
        print('   fwd %-40s rel-L2 %.2e' % (what, e))
        assert e <= HEAD_TOL, what
        assert torch.equal(zbuf[N:], ztail), 'fwd wrote past z[N]: ' + what
        if not use_b:
            continue                      # the backward does not read b
        # backward: dx overwrites, dw / db accumulate
        dx_ref = gz.double()[:, None] * m64 * w.double()[None, :]
        dw_ref = dw0.double() + (gz.double()[:, None] * m64 * x.double()).sum(0)
        db_ref = db0.double() + gz.double().sum()
        for want_dx, want_dwb in ((True, False), (False, True), (True, True)):
            dxbuf, dx, dxtail = _guarded(N * n, fill=7.0)
            dwbuf, dw, dwtail = _guarded(dw0)
            dbbuf, db, dbtail = _guarded(db0)
            ops.dense_head_bwd(xd, md if use_mask else None, wd, gzd, N, n, dx=dx if want_dx else None, dw=dw if want_dwb else None,
                               db=db if want_dwb else None)
            which = what + ' dx %s dw+db %s' % (want_dx, want_dwb)
            if want_dx:
                assert rel_l2(dx, dx_ref) <= HEAD_TOL, which
            else:
                assert bool((dx == 7.0).all()), which
            if want_dwb:
                assert rel_l2(dw, dw_ref) <= HEAD_TOL and rel_l2(db, db_ref) <= HEAD_TOL, which
                # the gradient itself, not diluted by the old contents (one more rounding, of old + gradient: 2^-24 |old + gradient|)
                assert rel_l2(dw.double().cpu() - dw0.double(), dw_ref - dw0.double()) <= 1e-5 + 2.0 ** -23 * float(dw_ref.norm() / (dw_ref - dw0.double()).norm()), which
            else:
                assert torch.equal(dw.cpu(), dw0) and torch.equal(db.cpu(), db0), which
            assert torch.equal(dxbuf[N * n:], dxtail) and torch.equal(dwbuf[n:], dwtail) and torch.equal(dbbuf[1:], dbtail), 'guard: ' + which


def test_dense_head_rejects_bad_arguments():
    from van_gan_amd import ops
    from van_gan_amd._lib import VgError
    x = torch.ones(2, 8, device=DEV); w = torch.ones(8, device=DEV); gz = torch.ones(2, device=DEV); z = torch.full((2,), 7.0, device=DEV)
    with pytest.raises(VgError):
        ops.dense_head_bwd(x, None, w, gz, 2, 8)                    # no output at all
    with pytest.raises(VgError):
        ops.dense_head_fwd(x, None, w, None, 0, 8, z)
    with pytest.raises(VgError):
        ops.dense_head_fwd(x, None, None, None, 2, 8, z)
    torch.cuda.synchronize()
    assert bool((z == 7.0).all())


@pytest.mark.parametrize('B', [1, 2, 3])
def test_wasserstein_terms(B):
    """acc2 += (sum z_real, sum z_fake); gz_d = (-inv x B, +inv x B); gz_g = -inv x B, each optional.  The gradients are constants: exact.
    The sums are B + 1 fp32 additions: |error| <= (B + 1) 2^-24 (|old| + sum |z|)."""
    from van_gan_amd import ops
    g = torch.Generator().manual_seed(40 + B)
    z = _rand(g, 2 * B, signed=True)
    acc0 = _rand(g, 2, signed=True)
    inv = 1.0 / (B * 3)
    inv32 = float(np.float32(inv))
    ref = acc0.double() + torch.stack([z[:B].double().sum(), z[B:].double().sum()])
    tol = (B + 1) * 2.0 ** -24 * (acc0.double().abs() + torch.stack([z[:B].double().abs().sum(), z[B:].double().abs().sum()]))
    zd = z.to(DEV)
    for want_d, want_g in ((True, True), (True, False), (False, True), (False, False)):
        accbuf, acc, acctail = _guarded(acc0)
        dbuf, gz_d, dtail = _guarded(2 * B, fill=7.0)
        gbuf, gz_g, gtail = _guarded(B, fill=7.0)
        ops.wasserstein_terms(zd, B, inv, acc, gz_d=gz_d if want_d else None, gz_g=gz_g if want_g else None)
        which = 'B %d gz_d %s gz_g %s' % (B, want_d, want_g)
        assert bool(((acc.double().cpu() - ref).abs() <= tol).all()), (which, acc.cpu(), ref)
        want = torch.tensor([-inv32] * B + [inv32] * B, dtype=torch.float32) if want_d else torch.full((2 * B,), 7.0)
        assert torch.equal(gz_d.cpu(), want), which
        want = torch.tensor([-inv32] * B, dtype=torch.float32) if want_g else torch.full((B,), 7.0)
        assert torch.equal(gz_g.cpu(), want), which
        assert torch.equal(accbuf[2:], acctail) and torch.equal(dbuf[2 * B:], dtail) and torch.equal(gbuf[B:], gtail), 'guard: ' + which


# ------------------------------------------------------------------------------------------------------------------------------------
# db[c] += sum over rows of dy[row][c].  Three regimes of the block layout: C divides 256 (1, 8, 256); C does not (48, 96: 240 / 192 active
# lanes, the rest of the block idles); C > 256 (384: the channel-block loop).  rows = 1023 * 5 + 3 is more than the grid cap of 1023
# blocks times the 5 rows a block holds at C = 48, so blocks stride over rows; at C = 1 a block holds 256 rows and most of the last idles.
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('rows', [1, 5, 1023 * 5 + 3])
@pytest.mark.parametrize('C', [1, 8, 48, 96, 256, 384])
def test_bias_grad(C, rows, dtype):
    """rel-L2 <= 1e-5 against the float64 column sum of the same values (bf16 inputs are bf16 values: the sum itself is not rounded).
    fp32 accumulation over <= 5118 rows, in registers, through LDS and by one atomic per block and channel."""
    from van_gan_amd import ops
    from van_gan_amd._lib import check, lib
    g = torch.Generator().manual_seed(C * 7919 + rows)
    dy = (torch.randn(rows, C, generator=g) + 0.5).to(dtype)
    db0 = _rand(g, C, signed=True)
    dbbuf, db, tail = _guarded(db0)
    dyd = dy.to(DEV)
    check(lib.vg_bias_grad(dyd.data_ptr(), int(dtype == torch.float32), rows, C, db.data_ptr(), ops.stream()), 'vg_bias_grad')
    ref = db0.double() + dy.double().sum(0)
    e = rel_l2(db, ref)
    e_grad = rel_l2(db.double().cpu() - db0.double(), dy.double().sum(0))
    print('   C %3d rows %4d %s rel-L2 %.2e (gradient alone %.2e)' % (C, rows, dtype, e, e_grad))
    assert e <= 1e-5
    assert e_grad <= 1e-5 + 2.0 ** -23 * float(ref.norm() / dy.double().sum(0).norm())        # + the rounding of old + gradient
    assert torch.equal(dbbuf[C:], tail), 'wrote past db[C]'
    assert lib.vg_bias_grad(dyd.data_ptr(), int(dtype == torch.float32), 0, C, db.data_ptr(), ops.stream()) == -1
    assert lib.vg_bias_grad(dyd.data_ptr(), int(dtype == torch.float32), rows, 0, db.data_ptr(), ops.stream()) == -1


# ------------------------------------------------------------------------------------------------------------------------------------
# y = alpha a + beta b (+ y).  Callers: the data path and the windowed inference (2 n - 1), the inference's final 255 n, the clDice
# backward (accumulate).  None of them passes y = a, so aliasing is not asserted here.  n = 8192 * 256 + 3 is past the largest grid.
#
# Against float32 numpy in the same order.  Without b there is one multiplication and (accumulating) one addition: nothing to contract,
# the result is exact.  With b the compiler contracts alpha a + (beta b) into one fused multiply-add (the product alpha a is not rounded),
# so the device may differ from the two-rounding float32 result by the rounding of alpha a: at most one unit in the last place (one
# part in 2^23) of the larger of |alpha a| and the sum.  Where both products are exact -- the callers' alpha = 2, beta = -1, b = 1 --
# it is exact again.
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('n', [1, 257, 8192 * 256 + 3])
def test_axpby(n, accumulate):
    from van_gan_amd import ops
    rng = np.random.default_rng(n + int(accumulate))
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    y0 = rng.standard_normal(n).astype(np.float32)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ones = np.ones(n, dtype=np.float32)
    for alpha, beta, bb, exact in ((0.75, 0.0, None, True), (1.7, 0.0, None, True), (2.0, -1.0, ones, True), (1.7, -0.3, b, False)):
        al, be = np.float32(alpha), np.float32(beta)
        ybuf, y, tail = _guarded(torch.from_numpy(y0))
        ops.axpby(ad, alpha, None if bb is None else (bd if bb is b else torch.from_numpy(bb).to(DEV)), beta, y, accumulate=accumulate)
        v = al * a if bb is None else al * a + be * bb
        ref = y0 + v if accumulate else v
        got = y.cpu().numpy()
        which = 'n %d alpha %g beta %g b %s accumulate %s' % (n, alpha, beta, bb is not None, accumulate)
        if exact:
            assert np.array_equal(got, ref), (which, int((got != ref).sum()))
        else:
            tol = 2.0 ** -23 * np.maximum(np.abs(al * a), np.abs(v)).astype(np.float64)
            if accumulate:
                tol = tol + 2.0 ** -23 * np.abs(ref)                 # the addition of y rounds once more, on either side
            d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            print('   %s: %d of %d differ from the two-rounding result, largest %.2f of the allowance' % (which, int((d > 0).sum()), n, float((d / tol).max())))
            assert np.all(d <= tol), which
            # and against the exact value: a fused result is never further from it than one rounding of alpha a plus one of the result
            exact64 = al.astype(np.float64) * a.astype(np.float64) + (be * bb).astype(np.float64) + (y0.astype(np.float64) if accumulate else 0.0)
            assert np.all(np.abs(got - exact64) <= tol), which
        assert torch.equal(ybuf[n:], tail), 'wrote past y[n]: ' + which


@pytest.mark.parametrize('n,wg', [(4, 1), (4 * 1001, 3), (4 * 1001, 1024), (4 * 70000, 7)])
def test_local_exchange_is_the_identity(n, wg):
    """vg_local_exchange, the one-GPU stand-in for a gradient all-reduce: every workgroup copies its slice of buf to scratch and back, so
    buf ends bit-identical, scratch holds a copy, nothing behind either is written.  wg = 1024 > n / 4 slices: most workgroups own nothing."""
    from van_gan_amd import ops
    from van_gan_amd._lib import check, lib
    g = torch.Generator().manual_seed(n + wg)
    v = torch.randn(n, generator=g)
    bbuf, b, btail = _guarded(v)
    sbuf, s, stail = _guarded(n, fill=7.0)
    check(lib.vg_local_exchange(b.data_ptr(), s.data_ptr(), n, wg, 0, ops.stream()), 'vg_local_exchange')
    assert torch.equal(b.cpu(), v) and torch.equal(s.cpu(), v)
    assert torch.equal(bbuf[n:], btail) and torch.equal(sbuf[n:], stail)
    for bad in ((b.data_ptr(), s.data_ptr(), n + 2, wg, 0), (b.data_ptr(), s.data_ptr(), n, 0, 0), (b.data_ptr(), s.data_ptr(), n, 1025, 0),
                (b.data_ptr() + 4, s.data_ptr(), n, wg, 0), (b.data_ptr(), None, n, wg, 0), (b.data_ptr(), s.data_ptr(), n, wg, 100001)):
        assert lib.vg_local_exchange(*bad, ops.stream()) == -1, bad
