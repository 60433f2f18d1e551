"""The N > 1 path on DISTINCT physical devices over RCCL (`nccl` backend) -- skipped unless the box shows at least two GPUs (the build's
boxes have one; tests/test_hip_dist.py runs the same code with the ranks sharing a GPU over gloo, tests/test_dist_gloo.py on CPU).

What the first collective between two MI355X must show (reference counterpart: torch.nn.DataParallel's scatter / gather around one backward,
src/Trainer01.py:517; the losses are means over their row classes, loss_functions/MSE01.py:55-59):

  * vdist.verify_sharded_gradient -- every rank's shard of one global batch (nerf + sparse-depth rows, split per class), shard gradients
    all-reduced with ReduceOp.AVG, against the whole batch's gradient computed locally by every rank: rel L2 <= 1e-5;
  * every rank's fine depths are the global rows' (Philox keyed by global ray index);
  * after K steps of sharded training the ranks' parameters are bit-identical (vdist.params_identical);
  * a frame rendered as R strips, one per device, is the frame one device renders, bit for bit;
  * `bench.py --gpus R` itself: exit status 0 and the line's grad_allreduce_vs_whole_batch / ranks_param_identical fields.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'vip-nerf_amd'), os.path.join(ROOT, 'vip-nerf_amd', 'src'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

N_DEV = torch.cuda.device_count() if torch.cuda.is_available() else 0
pytestmark = pytest.mark.gpu
needs_two = pytest.mark.skipif(N_DEV < 2, reason='needs at least two GPUs (one rank per physical device over RCCL)')
WORLDS = [w for w in (2, 4, 8) if w <= N_DEV]
N_NERF, N_SD, STEPS = 768, 256, 3


def _env(rank, world, port):
    if world == 1:
        os.environ['VIPNERF_FORCE_DIST'] = '1'           # one rank: the collectives still run (RCCL at world size 1)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      VIPNERF_DIST_BACKEND='nccl', HSA_ENABLE_IPC_MODE_LEGACY='0')


def _worker(rank, world, port, ret):
    _env(rank, world, port)
    from oracle import vipnerf_oracle as vo                      # (checker side: the synthetic batch and the initial weights)
    from loss_functions.LossComputerHip01 import LossComputerHip
    from vipnerf_hip import dist as vdist
    from vipnerf_hip.optim import FlatAdam
    import test_hip_parity as tp
    r, w, local = vdist.init_from_env()
    assert torch.distributed.get_backend() == 'nccl' and (r, w) == (rank, world)
    dev = torch.device(f'cuda:{local}')
    torch.cuda.set_device(dev)
    b = vo.synthetic_batch(N_NERF, 11, scene='realestate', nf=3, n_sparse=N_SD)
    gb = tp.ref_batch(b, dev, 40000)
    model, cfg = tp.make_model(dev, True, vo.init_params(20 + rank, scale=1.6), sparse=True)      # different on purpose: the broadcast fixes it
    vdist.broadcast_parameters(model, src=0)
    model.train()
    lossc = LossComputerHip(cfg)
    bucket = vdist.FlatGradBucket(model.parameters())
    z = {}

    def grad_fn(batch):
        bb = dict(batch)
        bb['common_data'] = {'poses': batch['common_data']['poses']}
        model.injected_rng = {'offset': 40000 << 16}
        try:
            bucket.release()
            out = model(bb)
            lossc.compute_losses(bb, out)['TotalLoss'].backward()
        finally:
            model.injected_rng = None
        z['shard' if 'rng_ray_ids' in batch else 'whole'] = out['z_vals_fine'].detach()
        flat = bucket.adopted()
        assert flat is not None and flat.numel() == 1191946
        return flat

    res = vdist.verify_sharded_gradient(grad_fn, gb, r, w)
    ids = vdist.shard_row_ids(gb, r, w)
    res['depths_are_the_global_rows'] = bool(torch.equal(z['shard'], z['whole'][ids]))
    # K sharded training steps: identical weights, one all-reduce of the flat bucket, the same Adam step everywhere
    opt = FlatAdam(model.parameters(), lr=5e-4, betas=(0.9, 0.999))
    for it in range(STEPS):
        bb = vdist.shard_batch(tp.ref_batch(vo.synthetic_batch(N_NERF, 50 + it, scene='realestate', nf=3, n_sparse=N_SD), dev, 40001 + it), r, w)
        bucket.release()
        out = model(bb)
        lossc.compute_losses(bb, out)['TotalLoss'].backward()
        bucket.all_reduce_mean()
        opt.step()
    res['params'] = vdist.params_identical(model.parameters())
    ret[rank] = res
    vdist.barrier()
    torch.distributed.destroy_process_group()


@needs_two
@pytest.mark.parametrize('world', WORLDS)
def test_reduced_shard_gradients_equal_the_whole_batch_gradient(world):
    port = 35000 + (os.getpid() % 2000) + world
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    for r in range(world):
        res = ret[r]
        print(f'world {world} rank {r}: reduced vs whole-batch gradient rel L2 {res["rel_l2_rank"]:.2e} (max over ranks {res["rel_l2"]:.2e}, bound 1e-5)')
        assert res['ranks'] == world and res['rel_l2'] <= 1e-5, res
        assert res['depths_are_the_global_rows'], f'rank {r}: fine depths differ from the global rows\' (Philox by global ray index)'
        assert res['params']['identical'], f'rank {r}: parameters differ from rank 0\'s after {STEPS} steps: {res["params"]}'


def _strip_worker(rank, world, port, ret):
    _env(rank, world, port)
    from vipnerf_hip import dist as vdist
    from data_preprocessors.RayGeneratorHip01 import predict_frame_sharded
    import test_hip_dist as thd
    r, w, local = vdist.init_from_env()
    dev = torch.device(f'cuda:{local}')
    torch.cuda.set_device(dev)
    model, gen = thd._render_setup(dev)
    full = predict_frame_sharded(model, gen, frame=1, rank=r, world=w)
    ret[rank] = {k: v.cpu().numpy() for k, v in full.items()}          # (world size 1 returns the strip on the device)
    torch.distributed.destroy_process_group()


@needs_two
@pytest.mark.parametrize('world', WORLDS)
def test_frame_as_one_strip_per_device_equals_one_device(world):
    from data_preprocessors.RayGeneratorHip01 import predict_frame
    import test_hip_dist as thd
    port = 37000 + (os.getpid() % 2000) + world
    ret = mp.Manager().dict()
    mp.spawn(_strip_worker, args=(world, port, ret), nprocs=world, join=True)
    model, gen = thd._render_setup(torch.device('cuda:0'))
    whole = predict_frame(model, gen, frame=1)
    for r in range(world):
        for k, v in whole.items():
            assert np.array_equal(ret[r][k], v.cpu().numpy()), f'world {world} rank {r}: {k}'


@needs_two
def test_bench_line_verifies_itself_on_distinct_devices():
    world = WORLDS[-1]
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'VIPNERF_DIST_BACKEND')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(world), '--steps', '3', '--warmup', '1', '--rays', '1024',
                        '--full', '--no-configs4', '--no-configs2', '--no-render', '--repeats', '1'], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][0])
    assert res['n_gpus'] == world and res['ranks_reduced'] == world
    assert 0 <= res['grad_allreduce_vs_whole_batch'] <= 1e-5 and res['ranks_param_identical'] is True
    assert res['allreduce_ms_per_step'] > 0


def test_the_workers_run_with_one_rank_over_rccl():
    """The box this suite usually sees has ONE device, so the tests above are skipped there -- their worker code must not meet a real node untested:
    the same two workers with world size 1 over RCCL (forced collectives): every line of them executes, the checks hold trivially."""
    port = 38000 + (os.getpid() % 2000)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(1, port, ret), nprocs=1, join=True)
    res = ret[0]
    assert res['ranks'] == 1 and res['rel_l2'] <= 1e-7 and res['depths_are_the_global_rows'] and res['params']['identical'], res
    ret2 = mp.Manager().dict()
    mp.spawn(_strip_worker, args=(1, port + 1, ret2), nprocs=1, join=True)
    assert ret2[0]['image'].dtype == np.uint8
