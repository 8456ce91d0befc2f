"""Workspaces at exactly the size the library asks for: the case lists and the host-side boundary search.

vg_conv3d plans with the caller's vg_conv_desc::scratch_bytes, vg_conv3d_wgrad with its scratch_bytes argument; every other test hands
both far more than any plan needs (ops.CONV_SCRATCH_BYTES: 160 MB, ops.WGRAD_SCRATCH_ELEMS: 384 MB), so a kernel that used more than its
host formula grants would have megabytes of silence behind it.  Here the smallest workspace that still yields the roomy plan is searched
on the CPU, with the dry run of the dispatch (ops.DryRun: vg_conv3d_variant / vg_conv3d_wgrad_variant) under a stand-in for
ops.conv_scratch / a pre-seeded ops.WGRAD_SCRATCH, and compared with the size recomputed from the plan:

  gather K split (conv<...>|ks>=2)   VG_SCRATCH_CTR_BYTES + cells * ks * (voxels per tile * BN * 4): one fp32 partial tile per cell and
                                     slice, cells = tiles * channel panels * N, all three from vg_conv3d_plan
  conv_dma (wlayout != 0)            vg_conv3d_scratch_bytes(d) for the roomy plan; VG_SCRATCH_CTR_BYTES + the operand (that value
                                     minus the partial tiles of its K split) is the floor below which vg_conv3d returns VG_EINVAL

tests/test_containment_host.py checks the search on the CPU; tests/test_gpu_containment.py launches at the sizes found, inside guards.

Helper module (no tests in here)."""
from __future__ import annotations

import ctypes as C
import functools
import re
from typing import Dict, List, Optional, Tuple

import torch

import layer_recipes as LR

CTR = 16384             # VG_SCRATCH_CTR_BYTES of include/vangan_hip.h (tests/test_containment_host.py compares it with the binding's)
ROOMY = CTR + (160 << 20)


class Workspace:
    """Stands in for ops.conv_scratch while active: every vg_conv3d descriptor gets `nbytes` bytes at `tensor` (a dummy address in a dry
    run; nbytes None: no workspace at all, scratch = NULL) instead of the stream's 160 MB buffer.  Notes, per descriptor, the tile plan
    (vg_conv3d_plan), wlayout and what vg_conv3d_scratch_bytes asks for."""

    def __init__(self, nbytes: Optional[int], tensor: Optional[torch.Tensor] = None):
        assert tensor is None or (nbytes is not None and tensor.numel() * tensor.element_size() >= nbytes)
        self.nbytes, self.tensor, self.seen = nbytes, tensor, []

    def __call__(self, d, s_, device=None):
        from van_gan_amd import _lib
        plan = (C.c_int32 * 4)()
        rc = _lib.lib.vg_conv3d_plan(C.byref(d), plan)
        self.seen.append(dict(plan=tuple(plan) if rc == 0 else None, wlayout=int(d.wlayout), need=int(_lib.lib.vg_conv3d_scratch_bytes(C.byref(d)))))
        if self.nbytes is None:
            d.scratch, d.scratch_bytes = None, 0
        elif self.tensor is None:
            d.scratch, d.scratch_bytes = 1 << 20, self.nbytes
        else:
            d.scratch, d.scratch_bytes = self.tensor.data_ptr(), self.nbytes

    def __enter__(self):
        from van_gan_amd import ops
        self._saved, ops.conv_scratch = ops.conv_scratch, self
        return self

    def __exit__(self, *exc):
        from van_gan_amd import ops
        ops.conv_scratch = self._saved
        return False


def variant_at(call, nbytes: Optional[int]) -> Tuple[Optional[str], Workspace]:
    """(the one variant `call` (layer_recipes.empty_call) selects with an nbytes-byte workspace, or None if the library refuses the call
    (VG_EINVAL); the Workspace with what it noted)."""
    with Workspace(nbytes) as ws:
        try:
            got = LR.dry_variants(call)
        except RuntimeError:
            return None, ws
    assert len(set(got)) == 1, got
    return got[0], ws


def smallest_keeping(variant_of, roomy: int, want: str, granule: int = 1) -> int:
    """The smallest multiple of `granule` for which variant_of(nbytes) == want, by bisection between 0 and `roomy` (where it holds).  The
    caller checks the two properties a bisection of a non-monotone function would not give: the plan at one granule less differs."""
    assert roomy % granule == 0 and variant_of(roomy) == want
    lo, hi = -1, roomy // granule               # variant_of(lo * granule) != want (below zero by convention), variant_of(hi * granule) == want
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if variant_of(mid * granule) == want:
            hi = mid
        else:
            lo = mid
    return hi * granule


# ----------------------------------------------------------------------------------------------------------------------
# the representative lists' cases
# ----------------------------------------------------------------------------------------------------------------------
def _all_reps() -> List[Tuple[str, Tuple[str, str], dict]]:
    out = []
    for name, reps in (('layers', LR.representatives()), ('inference', LR.inference_representatives()), ('ragged', LR.ragged_representatives()),
                       ('batch3', LR.batch3_representatives())):
        out += [(name, kv, r) for kv, r in reps.items()]
    return out


def ks_of(variant: str) -> int:
    m = re.search(r'\|ks(\d+)', variant)
    return int(m.group(1)) if m else 0


@functools.lru_cache(maxsize=None)
def ksplit_cases() -> Dict[str, dict]:
    """case id -> {'kind', 'variant', 'recipe', 'list', ...}: one per distinct gather K-split variant (conv<...>|ks>=2) of the four
    representative lists -- the cheapest call over the lists that selects it."""
    best: Dict[Tuple[str, str], dict] = {}
    for name, kv, r in _all_reps():
        if kv[1].startswith('conv<') and ks_of(kv[1]) >= 2 and (kv not in best or r['macs'] < best[kv]['macs']):
            best[kv] = dict(kind=kv[0], variant=kv[1], recipe=r['recipe'], list=name, config=r['config'], layer=r['layer'], macs=r['macs'])
    return {'%s %s' % kv: c for kv, c in sorted(best.items())}


def ksplit_expected(variant: str, plan) -> int:
    """VG_SCRATCH_CTR_BYTES + cells * ks * one fp32 partial tile, from the plan vg_conv3d_plan reports: plan[0] channels per panel,
    plan[1] voxels per tile, plan[3] = tiles * panels * N cells."""
    return CTR + plan[3] * ks_of(variant) * plan[1] * plan[0] * 4


@functools.lru_cache(maxsize=None)
def ksplit_boundary(cid: str) -> dict:
    """Host side of one K-split case: S (smallest workspace that keeps the variant), the size recomputed from the plan, and the variants
    at S - 16 and without a workspace."""
    c = ksplit_cases()[cid]
    call = LR.empty_call(c['recipe'])
    roomy, ws = variant_at(call, ROOMY)
    assert roomy == c['variant'], (roomy, c['variant'])
    plan = ws.seen[-1]['plan']
    S = smallest_keeping(lambda n: variant_at(call, n)[0], ROOMY, roomy)
    return dict(S=S, expected=ksplit_expected(roomy, plan), plan=plan, below=variant_at(call, S - 16)[0], none=variant_at(call, None)[0])


@functools.lru_cache(maxsize=None)
def dma_cases() -> Dict[str, dict]:
    """case id -> case: the conv_dma calls (descriptors with wlayout != 0), forward and data gradient.  For each distinct (kind, layer
    constructor) of the lists the call on the smallest grid, and that call again with N = 1, 2 and 3 samples."""
    best: Dict[tuple, dict] = {}
    for name, kv, r in _all_reps():
        if not kv[1].startswith('conv_dma') or kv[0] == 'wgrad':
            continue
        L = r['recipe']['layer']
        key = (kv[0], L['k'], L['cin'], L['cout'], L['stride'], L['pad'])
        vox = L['in_dims'][0] * L['in_dims'][1] * L['in_dims'][2]
        if key not in best or (vox, r['macs']) < best[key]['order']:
            best[key] = dict(order=(vox, r['macs']), recipe=r['recipe'], list=name, config=r['config'], layer=r['layer'])
    cases = {}
    for key, b in sorted(best.items()):
        for N in (1, 2, 3):
            r = b['recipe']
            r = dict(r, src=dict(r['src'], N=N)) if 'src' in r else dict(r, N=N)
            if r.get('fin'):
                r = dict(r, fin=None)
            cid = '%s k%d %d->%d s%d %s %s N%d' % (key + ('x'.join(str(n) for n in r['layer']['in_dims']), N))
            cases[cid] = dict(kind=key[0], recipe=r, list=b['list'], config=b['config'], layer=b['layer'])
    return cases


@functools.lru_cache(maxsize=None)
def dma_boundary(cid: str) -> dict:
    """Host side of one conv_dma case: the roomy variant, what vg_conv3d_scratch_bytes asks for (`need`), the smallest workspace that
    keeps the roomy variant (S), the smallest the library accepts at all (`floor`) and the variants around both."""
    c = dma_cases()[cid]
    call = LR.empty_call(c['recipe'])
    roomy, ws = variant_at(call, ROOMY << 3)
    assert roomy is not None and roomy.startswith('conv_dma'), roomy
    assert len(ws.seen) == 1 and ws.seen[0]['wlayout'] != 0
    need = ws.seen[0]['need']
    at = lambda n: variant_at(call, n)[0]
    S = smallest_keeping(at, ROOMY << 3, roomy)
    floor = smallest_keeping(lambda n: at(n) is not None, ROOMY << 3, True)
    return dict(roomy=roomy, need=need, S=S, floor=floor, at_need=at(need), below_S=at(S - 1), at_floor=at(floor), below_floor=at(floor - 1))


# ----------------------------------------------------------------------------------------------------------------------
# weight gradients: the scratch argument of vg_conv3d_wgrad
# ----------------------------------------------------------------------------------------------------------------------
WGRAD_ROOMY = (96 << 20) * 4            # ops.WGRAD_SCRATCH_ELEMS floats
WGRAD_GRANULE = 4                       # ops passes sc.numel() * 4: one float


class _FakeScratch:
    """What ops.ConvLayer._wgrad asks of its scratch tensor, without memory behind it: for dry runs."""

    def __init__(self, nbytes):
        self.n = nbytes // 4

    def numel(self):
        return self.n

    def data_ptr(self):
        return 0x1000 if self.n else 0


class WgradWorkspace(dict):
    """Stands in for ops.WGRAD_SCRATCH while active: whatever (device, stream) asks, it gets `tensor` -- a float32 view of exactly the
    bytes under test (None: a dry run, a stand-in of nbytes bytes without memory; nbytes 0: no workspace, the pointer is NULL)."""

    def __init__(self, nbytes: int, tensor: Optional[torch.Tensor] = None):
        super().__init__()
        assert nbytes % WGRAD_GRANULE == 0 and (tensor is None or (tensor.dtype == torch.float32 and tensor.numel() * 4 == nbytes))
        self.sc = _FakeScratch(nbytes) if tensor is None else tensor

    def get(self, key, default=None):
        return self.sc

    def __enter__(self):
        from van_gan_amd import ops
        self._saved, ops.WGRAD_SCRATCH = ops.WGRAD_SCRATCH, self
        return self

    def __exit__(self, *exc):
        from van_gan_amd import ops
        ops.WGRAD_SCRATCH = self._saved
        return False


def wgrad_variant_at(call, nbytes: int) -> str:
    with WgradWorkspace(nbytes):
        got = LR.dry_variants(call)
    assert len(got) == 1, got
    return got[0]


@functools.lru_cache(maxsize=None)
def wgrad_cases() -> Dict[str, dict]:
    """family -> case: for each weight-gradient kernel family whose plan depends on the workspace (the roomy plan differs from the one
    without a workspace: wgrad_thin, wgrad_dma, wgrad_pw_dma, c1m_wgrad's and the generic kernel's partial slabs, ...), the cheapest
    call of the representative lists, with S (the smallest workspace, in floats' bytes, that keeps the roomy variant) and the variants
    at S, one float less and none."""
    best: Dict[str, dict] = {}
    for name, kv, r in _all_reps():
        if kv[0] != 'wgrad':
            continue
        fam = kv[1].split('<')[0]
        if fam in best and best[fam]['macs'] <= r['macs']:
            continue
        call = LR.empty_call(r['recipe'])
        roomy, none = wgrad_variant_at(call, WGRAD_ROOMY), wgrad_variant_at(call, 0)
        assert roomy == kv[1], (roomy, kv[1])
        if roomy != none:
            best[fam] = dict(recipe=r['recipe'], list=name, config=r['config'], layer=r['layer'], macs=r['macs'], roomy=roomy, none=none, call=call)
    for c in best.values():
        at = lambda n, call=c['call']: wgrad_variant_at(call, n)
        c['S'] = smallest_keeping(at, WGRAD_ROOMY, c['roomy'], WGRAD_GRANULE)
        c['below'] = at(c['S'] - WGRAD_GRANULE)
    return best
