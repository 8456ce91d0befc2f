"""The real engine under world_size 2 on ONE GPU (both ranks on cuda:0, gloo process group -- RCCL refuses two ranks on one
device): exercises what the driver's multi-GPU runs do on the product path -- rank-0 weight broadcast, the four per-network
gradient all-reduces issued from the two stream lanes onto the communication stream, Adam on the reduced buckets, SUM of the
result dict -- and checks the data-parallel semantics of the reference (MirroredStrategy, vangan.py:426-438,472-490;
loss_functions.py:7-22,226): every replica computes its losses on its LOCAL batch with the GLOBAL batch size in the
denominators and lambda_topology / n_devices on the clDice term; gradients and result scalars are SUMMED.  (Note that this is
NOT the same as one process with the two samples as a batch: the reference's reduce_mean(axis=None) terms -- cycle BCE, SSIM
reconstruction -- average over the local batch before dividing by the global batch size, and clDice is a ratio of sums.)

Expected values come from the same engine run as "rank r of 2" without a process group (n_devices=2, one sample, apply=False):
gradients summed on the host, then one Adam step.  Exact-parity mode (fp32 storage), dropout/noise off.  Tolerances: only fp32
summation orders differ (float atomics): losses rel 1e-4; updated weights: <= 0.2 % of the elements differ by more than 1e-4
(Adam's first step is sign-like, so a ~0 gradient that flips sign moves a weight by 2*lr = 4e-4)."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (32, 32, 32)

WORKER = r'''
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
from van_gan_amd.vangan import VanGan
from oracle.vangan_oracle import synth_volumes
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
backend = os.environ['VG_TEST_BACKEND']
dev = 'cuda:%%d' %% (rank if backend == 'nccl' else 0)       # RCCL: one device per rank; gloo: both ranks on cuda:0
torch.cuda.set_device(dev)
if backend == 'nccl':
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device(dev))
else:
    dist.init_process_group('gloo', rank=rank, world_size=world)
eng = VanGan(%(dims)r, batch_size=1, n_devices=world, device=dev, seed=rank * 17, layer_noise=0.0, dropout_rate=0.0,
             process_group=dist.group.WORLD, precision='fp32')
eng.broadcast_weights(0)
rI, rS = synth_volumes(2, *%(dims)r, seed=5)
res = None
for _ in range(1):
    res = eng.distributed_train_step(rI[rank:rank + 1].to(dev), rS[rank:rank + 1].to(dev))
torch.cuda.synchronize()
# the stochastic layers of two replicas must not share a stream (discriminator.py:52,108 under MirroredStrategy): same seed on
# both ranks here, different Philox keys
eng2 = VanGan(%(dims)r, batch_size=1, n_devices=world, device=dev, seed=0, process_group=dist.group.WORLD)
nz, dp = eng2._make_noise(eng2.disc_S, 2, eng2.arena)
torch.cuda.synchronize()
torch.save({'w': {k: s.w.cpu() for k, s in eng.stores.items()}, 'res': res, 'noise_key': eng2.noise_key,
            'noise': nz['down2'].float().cpu(), 'drop': dp['down2'].cpu()}, %(out)r %% rank)
dist.destroy_process_group()
'''


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
def test_two_ranks_equal_one_process_with_batch_two(tmp_path, backend):
    if backend == 'nccl' and torch.cuda.device_count() < 2:
        pytest.skip('RCCL needs one device per rank: runs on boxes with >= 2 GPUs')
    from oracle.vangan_oracle import synth_volumes
    from van_gan_amd.vangan import VanGan
    out = str(tmp_path / 'rank%d.pt')
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % dict(root=ROOT, dims=DIMS, out=out))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0', VG_TEST_BACKEND=backend)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill(); o, _ = p.communicate()
        logs.append(o.decode()[-3000:])
    assert all(p.returncode == 0 for p in procs), '\n'.join(logs)
    a, b = torch.load(out % 0), torch.load(out % 1)
    # every rank applied the same update
    for k in a['w']:
        ne = a['w'][k] != b['w'][k]
        assert not bool(ne.any()), '%s: %d of %d weights differ between the ranks, max |diff| %.3e' % (
            k, int(ne.sum()), ne.numel(), float((a['w'][k] - b['w'][k]).abs().max()))
    assert a['res'] == b['res']
    # per-replica noise / dropout streams: different keys, uncorrelated draws of the expected spread
    assert a['noise_key'] != b['noise_key']
    na, nb = a['noise'].flatten(), b['noise'].flatten()
    assert not torch.equal(na, nb)
    corr = float((na * nb).mean() / (na.std() * nb.std()))
    assert abs(corr) < 0.02 and abs(float(na.std()) - 0.1) < 5e-3, (corr, float(na.std()))
    assert not torch.equal(a['drop'], b['drop'])
    # expectation: the same engine as "rank r of 2", no process group; gradients summed by hand
    eng = VanGan(DIMS, batch_size=1, n_devices=2, device='cuda:0', seed=0, layer_noise=0.0, dropout_rate=0.0, precision='fp32')
    rI, rS = synth_volumes(2, *DIMS, seed=5)
    gsum, rsum = None, None
    for r in range(2):
        res = eng.train_step(rI[r:r + 1].cuda(), rS[r:r + 1].cuda(), apply=False)
        g = {k: s.g.clone() for k, s in eng.stores.items()}
        gsum = g if gsum is None else {k: gsum[k] + g[k] for k in g}
        rsum = res if rsum is None else {k: rsum[k] + res[k] for k in res}
    for k, s in eng.stores.items():
        s.g.copy_(gsum[k])
    eng._apply_adam()
    torch.cuda.synchronize()
    for k, v in rsum.items():
        assert abs(a['res'][k] - v) <= 1e-4 * abs(v) + 1e-6, (k, a['res'][k], v)
    bad = tot = 0
    for k, s in eng.stores.items():
        d = (s.w.cpu() - a['w'][k]).abs()
        bad += int((d > 1e-4).sum()); tot += d.numel()
    assert bad <= 2e-3 * tot, (bad, tot)


RCCL_ONE = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
from van_gan_amd.vangan import VanGan
from van_gan_amd.synth import synth_volumes
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda:0'))
assert dist.get_backend() == 'nccl'
eng = VanGan(%(dims)r, batch_size=1, n_devices=1, device='cuda:0', seed=4, layer_noise=0.0, dropout_rate=0.0,
             process_group=dist.group.WORLD, precision='fp32')
assert eng.sync.active and eng.sync.forced and not eng.sync.fake and eng._xstep
eng.broadcast_weights(0)                                   # ncclBroadcast of the four weight buffers
rI, rS = synth_volumes(1, *%(dims)r, seed=5)
rI, rS = rI.cuda(), rS.cuda()
res = []
for _ in range(3):
    res.append(eng.distributed_train_step(rI, rS))         # ncclAllReduce: 4 buckets (two in two pieces) + the result scalars
eng._join_updates()
torch.cuda.synchronize()
torch.save({'w': {k: s.w.cpu() for k, s in eng.stores.items()}, 'res': res}, %(out)r)
dist.destroy_process_group()
"""


def test_rccl_process_group_of_one_rank_runs_the_collectives(tmp_path):
    """What a 1-GPU box can execute of the RCCL path: torch.distributed 'nccl' (= RCCL on ROCm) with ONE rank and VG_DDP_FORCE=1, so
    that GradSync issues every collective of the data-parallel step for real -- communicator set-up, rank-0 ncclBroadcast of the
    weights, ncclAllReduce of the four flat buckets on the engine's optimizer stream (pieces, per-bucket events, cross-step mode),
    the SUM of the result dict -- through the same code the 8-GPU job runs.  A SUM over one rank is the identity: three steps must
    give the weights and losses of an engine without a process group (exact-parity mode, stochastic layers off; only float-atomic
    summation orders differ -- tolerances as in the two-rank test)."""
    from van_gan_amd.synth import synth_volumes
    from van_gan_amd.vangan import VanGan
    out = str(tmp_path / 'rccl1.pt')
    script = tmp_path / 'rccl_one.py'
    script.write_text(RCCL_ONE % dict(root=ROOT, dims=DIMS, out=out))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0', VG_DDP_FORCE='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'VG_FAKE_AR'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    a = torch.load(out)
    eng = VanGan(DIMS, batch_size=1, n_devices=1, device='cuda:0', seed=4, layer_noise=0.0, dropout_rate=0.0, precision='fp32')
    rI, rS = synth_volumes(1, *DIMS, seed=5)
    rI, rS = rI.cuda(), rS.cuda()
    for i in range(3):
        res = eng.train_step(rI, rS)
        # step 0 sees identical weights (only float-atomic summation orders differ); every further step sits behind sign-like Adam updates of
        # 2e-4 per weight that a ~0 gradient's sign decides, so the two runs drift apart step by step: the third step's cycle loss differed
        # by 1.06 % in 1 of 7 runs (the others <= 0.5 %), hence the stated bound per step
        tol = (1e-4, 1e-2, 5e-2)[i]
        for k, v in res.items():
            assert abs(a['res'][i][k] - v) <= tol * abs(v) + 1e-5, (i, k, a['res'][i][k], v)
    torch.cuda.synchronize()
    bad = tot = 0
    for k, s in eng.stores.items():
        d = (s.w.cpu() - a['w'][k]).abs()
        bad += int((d > 1.5e-3).sum()); tot += d.numel()      # three sign-like Adam steps of 2e-4: a ~0 gradient that flips sign moves 4e-4 per step
    assert bad <= 1e-2 * tot, (bad, tot)


def test_bench_two_ranks_completes():
    """`python bench.py --gpus 2 --full` (bench.py starts its own one-process-per-GPU job as a child process; both ranks on
    cuda:0 over gloo here, VG_BENCH_ONE_DEVICE=1): the driver's multi-GPU contract -- barrier-bracketed timed steps, MAX over
    ranks, the per-launch timing step on EVERY rank (it contains the all-reduces: on rank 0 alone it dead-locked), one JSON
    line from rank 0, the child's return code relayed."""
    import json
    env = dict(os.environ, VG_BENCH_ONE_DEVICE='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--size', '32', '--full']
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    lines = [l for l in out.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out[-3000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 2 and d['scaling'] == 'weak' and d['value'] > 0
    assert d['roofline'] is not None and d['cpu_baseline'] is None
    assert d['config']['parallelism'] == 'dp2'


def test_weights_loaded_behind_an_unsynchronised_step_are_not_overwritten(tmp_path):
    """Cross-step mode (train_step(sync=False): Adam + repack of the step are still queued on the optimizer stream when the call
    returns).  load_checkpoint / load_weights / broadcast_weights right behind such a step must leave exactly the loaded values
    in the stores AND in the packed kernel weights -- the queued update must not land on top of them (vangan.py:252-268: the
    reference restores into idle variables).  Checked on a process group of one rank so that broadcast_weights runs too."""
    import torch.distributed as dist
    from oracle.vangan_oracle import synth_volumes
    from van_gan_amd.vangan import VanGan
    dist.init_process_group('gloo', rank=0, world_size=1, init_method='tcp://127.0.0.1:%d' % _free_port())
    try:
        eng = VanGan(DIMS, batch_size=1, device='cuda:0', seed=3, output_dir=str(tmp_path), process_group=dist.group.WORLD)
        rI, rS = synth_volumes(1, *DIMS, seed=9)
        rI, rS = rI.cuda(), rS.cuda()
        eng.train_step(rI, rS)
        path = eng.save_checkpoint(0)
        ck = torch.load(path, map_location='cpu')
        ref = eng.test_step(rI, rS)                         # losses of the checkpointed weights
        for mode in ('checkpoint', 'weights', 'broadcast'):
            for _ in range(3):
                eng.train_step(rI, rS, sync=False)          # returns with the last update still in flight
            if mode == 'checkpoint':
                assert eng.load_checkpoint(1)
            elif mode == 'weights':
                for k, s in eng.stores.items():
                    s.step = ck[k]['step']
                eng.load_weights({k: {n: t.clone() for n, t in exp.items()} for k, exp in saved.items()})
            else:
                eng.train_step(rI, rS, sync=False)
                before = {k: s.w.clone() for k, s in eng.stores.items()}      # reads on the current stream: not ordered behind the update
                eng.broadcast_weights(0)                    # one rank: the weights of the finished step, repacked
                torch.cuda.synchronize()
                after = {k: s.w.clone() for k, s in eng.stores.items()}
                eng.train_step(rI, rS)                      # and the engine still steps
                assert all(torch.isfinite(after[k]).all() for k in after) and before.keys() == after.keys()
                continue
            torch.cuda.synchronize()
            for k, s in eng.stores.items():
                assert torch.equal(s.w.cpu(), ck[k]['w']), (mode, k)
            got = eng.test_step(rI, rS)                     # the PACKED weights are the loaded ones too
            for key, v in ref.items():
                assert abs(got[key] - v) <= 2e-2 * abs(v) + 1e-4, (mode, key, got[key], v)
            if mode == 'checkpoint':
                saved = eng.export_weights()
    finally:
        dist.destroy_process_group()
