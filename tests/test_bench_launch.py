"""bench.py as the scaling harness invokes it: ``python bench.py --gpus N`` must produce an N-rank number or fail.

CPU: the self-launch path (parent -> ``torch.distributed.run`` -> N ranks) under gloo, and the refusal when the
node has fewer GPUs than asked for.  GPU: the sharded step over a REAL RCCL communicator (world size 1 -- the
only RCCL world a one-GPU box offers), in both collective layouts, equals the single-process step."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')


def _run(*argv, env=None, timeout=300):
    e = dict(os.environ)
    e.pop('WORLD_SIZE', None)
    e.pop('RANK', None)
    e.pop('LOCAL_RANK', None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH, *argv], capture_output=True, text=True, timeout=timeout, env=e)


def test_bench_self_launch_reaches_n_ranks_under_gloo():
    r = _run('--gpus', '2', '--spawn-selftest')
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1, r.stdout                       # rank 0 alone prints
    out = json.loads(line[0])
    assert {k: out[k] for k in ('selftest', 'n_gpus', 'ranks_seen')} == {'selftest': True, 'n_gpus': 2, 'ranks_seen': [0, 1]}
    assert out['fallback'] == 'none' and out['graph_comm'] is True and [a['status'] for a in out['attempts']] == ['ok']


@pytest.mark.parametrize('fault', ['exit', 'hang'])
def test_bench_falls_back_when_a_rank_dies_or_hangs_in_its_first_capture(fault):
    """rank 1's worker exits non-zero (or hangs) in its first attempt -- the rank supervisors stop every
    worker, agree through the launcher's store and start FRESH workers with NEMO_GRAPH_COMM=0; the parent still prints
    exactly one valid line, which says what happened."""
    r = _run('--gpus', '2', '--spawn-selftest', '--attempt-timeout', '8', env={'NEMO_TEST_FAIL_CAPTURE': fault}, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1, r.stdout
    out = json.loads(line[0])
    assert out['selftest'] and out['ranks_seen'] == [0, 1]
    assert out['fallback'] == 'NEMO_GRAPH_COMM=0' and out['graph_comm'] is False
    assert [a['status'] == 'ok' for a in out['attempts']] == [False, True]
    assert ('exit code 23' in out['attempts'][0]['status']) if fault == 'exit' else ('exceeded' in out['attempts'][0]['status'])


def test_bench_refuses_more_gpus_than_visible():
    have = torch.cuda.device_count()
    r = _run('--gpus', str(have + 1) if have else '2', '--steps', '1', '--warmup', '0')
    assert r.returncode == 3, (r.returncode, r.stderr[-500:])
    assert 'GPU(s) visible' in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith('{')]      # and no JSON line at all


def test_bench_rejects_world_size_mismatch():
    """Under a launcher (WORLD_SIZE set) the world must be what --gpus says -- in both directions."""
    r = _run('--gpus', '1', '--spawn-selftest', env={'WORLD_SIZE': '2', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode != 0 and 'WORLD_SIZE=2' in r.stderr
    r = _run('--gpus', '4', '--spawn-selftest', env={'WORLD_SIZE': '2', 'RANK': '0', 'LOCAL_RANK': '0'})
    assert r.returncode != 0 and 'WORLD_SIZE=2' in r.stderr


def test_step_flops_accounting():
    sys.path.insert(0, ROOT)
    import bench
    tot, parts = bench.step_flops(2400, skin_nnz=24)
    assert abs(parts['mesh'] - 69.649632e9) < 1e6           # the roofline kernel's algorithmic work
    sparse = bench.step_flops(2400, skin_nnz=4)[1]['mesh']   # 4 non-zero skinning weights per vertex: 2 x 48 of the 2 x 288
    assert abs(sparse - 2.0 * 2400 * 6890 * (2 * 3 * 207 + 2 * 48 + 288)) < 1e6 and bench.SKIN_NNZ == 4
    assert abs(parts['blend_adjoint'] - 20.54e9) < 0.01e9
    assert 120e9 < tot < 135e9


def test_dump_outputs_format_and_budget(tmp_path):
    """--dump-outputs: one .npy per returned array, float32 / float64 only; over 64 MB the per-sample arrays keep the SAME
    seeded rows in every run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from nemo_cvpr2023_amd.neural_motion_model import _LazyInfo
    n = 300000
    g = torch.Generator().manual_seed(0)

    def out():
        info = _LazyInfo({'view_idx': torch.arange(n) % 7, 'frame_idx': torch.arange(n) // 7})
        info.lazy.update(j=lambda: torch.randn(n, 45, 3, generator=torch.Generator().manual_seed(1)),
                         points2d=lambda: torch.randn(n, 45, 2, generator=torch.Generator().manual_seed(2)))
        return {'kp_loss': np.asarray(np.float32(1.5)), 'total_loss': np.asarray(np.float32(2.5))}, info
    small = bench.write_outputs(str(tmp_path / 'small'), {'total_loss': np.asarray(np.float32(2.5)),
                                                          'j': torch.randn(8, 3, generator=g).numpy()})
    assert small['sampled'] is None and small['files'] == ['j.npy', 'total_loss.npy']
    a = bench.write_outputs(str(tmp_path / 'a'), bench.host_outputs(out()))
    b = bench.write_outputs(str(tmp_path / 'b'), bench.host_outputs(out()))
    assert a['bytes'] <= bench.DUMP_BUDGET and a['sampled']['of'] == n and 0 < a['sampled']['rows'] < n
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in a['files']) <= bench.DUMP_BUDGET + 128 * len(a['files'])
    assert set(a['files']) == {'kp_loss.npy', 'total_loss.npy', 'view_idx.npy', 'frame_idx.npy', 'j.npy', 'points2d.npy',
                               'sample_rows.npy'}
    for f in a['files']:
        x, y = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    rows = np.load(tmp_path / 'a' / 'sample_rows.npy').astype(np.int64)
    full = torch.randn(n, 45, 3, generator=torch.Generator().manual_seed(1)).numpy()
    assert np.array_equal(np.load(tmp_path / 'a' / 'j.npy'), full[rows])
    assert np.array_equal(np.load(tmp_path / 'a' / 'frame_idx.npy'), rows // 7)


# ------------------------------------------------------------------------------------------ GPU
def _rccl_world1(mode, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from nemo_cvpr2023_amd import synthetic as syn
    from nemo_cvpr2023_amd.dist import ShardedNemo
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', init_method='tcp://127.0.0.1:%d' % q['port'], rank=0, world_size=1)
    assert dist.get_backend() == 'nccl'
    V, T, B = 3, 10, 16
    args = syn.published_args(h_dim=48, monotonic_network_n_nodes=20, batch_size=B, out_dir='', phase_rbf_dim=16)
    seqs = syn.SyntheticSequences(V, T, seed=1234)
    assets = dict(smpl_assets=syn.make_smpl_assets(128, seed=1), vposer_state=syn.make_vposer_state(),
                  gmm=syn.make_gmm())
    m = ShardedNemo(2, args, seqs, 'cuda:0', rank=0, world=1, seed=0, **assets)
    m.set_shard_mode(mode)
    g = torch.Generator().manual_seed(7)
    out = []
    for it in range(8):
        if it % 2:
            ld, _ = m.step(None, None, full_batch=True)
        else:
            ld, _ = m.step(torch.randint(0, V, (B,), generator=g), torch.randint(0, T, (B,), generator=g))
        out.append({k: float(v) for k, v in ld.items()})
    # the captured camera fit under RCCL (its capture must open thread-local while the process group's watchdog
    # thread is alive), twice with the global-trajectory switch toggled in between: the graph key must tell the two apart
    cam = [[float(x) for x in m.opt_cam(6)]]
    m.model.engine.start_global_traj_anywhere = not m.model.engine.start_global_traj_anywhere
    cam.append([float(x) for x in m.opt_cam(6)])
    m.model.engine.start_global_traj_anywhere = not m.model.engine.start_global_traj_anywhere
    q['cam'] = cam
    graphs = [v for w in m.model.engine.ws.values() for v in w['graphs'].values()]
    q['res'] = (out, sum(isinstance(x, torch.cuda.CUDAGraph) for x in graphs))
    del graphs
    m.close()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['single', 'split', 'buckets'])
def test_sharded_step_over_rccl_world_of_one(mode):
    """RCCL (backend 'nccl') on hardware: communicator creation, the all-reduce(s) of the sharded step on their
    streams, the watchdog thread next to HIP-graph capture and replay.  Numerically a 1-rank all-reduce is the
    identity, so the run must reproduce the plain single-process model."""
    import socket
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from nemo_cvpr2023_amd import synthetic as syn
    from nemo_cvpr2023_amd.neural_motion_model import NemoV2, make_init_state
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    q = {'port': s.getsockname()[1]}
    s.close()
    _rccl_world1(mode, q)
    got, n_graphs = q['res']
    assert n_graphs >= (0 if os.environ.get('NEMO_GRAPHS', '1') == '0' else 1)
    V, T, B = 3, 10, 16
    args = syn.published_args(h_dim=48, monotonic_network_n_nodes=20, batch_size=B, out_dir='', phase_rbf_dim=16)
    seqs = syn.SyntheticSequences(V, T, seed=1234)
    torch.manual_seed(0)
    state = make_init_state(args, 2, V, seqs.IMG_D0)
    m = NemoV2(args, seqs, 'cuda:0', smpl_assets=syn.make_smpl_assets(128, seed=1),
               vposer_state=syn.make_vposer_state(), gmm=syn.make_gmm())
    m.load_state_dict(state, strict=False)
    g = torch.Generator().manual_seed(7)
    for it in range(8):
        if it % 2:
            ld, _ = m.step(None, None, full_batch=True)
        else:
            ld, _ = m.step(torch.randint(0, V, (B,), generator=g), torch.randint(0, T, (B,), generator=g))
        for k, v in ld.items():
            assert abs(got[it][k] - float(v)) <= 1e-4 * max(abs(float(v)), 1e-6), (it, k, got[it][k], float(v))
    ref = [[float(x) for x in m.opt_cam(6)]]
    m.engine.start_global_traj_anywhere = not m.engine.start_global_traj_anywhere
    ref.append([float(x) for x in m.opt_cam(6)])
    for a, b in zip(q['cam'], ref):
        assert len(a) == len(b) == 6
        for x, y in zip(a, b):
            assert abs(x - y) <= 1e-4 * max(abs(y), 1e-6), (q['cam'], ref)
    assert ref[0] != ref[1]                                  # (the switch changes the objective: a stale graph would repeat run 1)


@pytest.mark.gpu
def test_bench_two_ranks_as_the_driver_launches_them(tmp_path):
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 ... bench.py --gpus 2 ...` -- the driver's own command
    line for the scaling run -- on the one GPU of this box (gloo instead of RCCL, which refuses two ranks per device):
    the whole N > 1 path of bench.py (world check, `--shard-mode auto` over all three layouts, the timed regions, the
    per-rank compute / collective probe, the sharded minibatch leg with padded launches, the roofline leg) must
    produce ONE JSON line with the contract's keys."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, NEMO_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), BENCH, '--gpus', '2', '--instances', '2', '--steps', '4', '--warmup', '1', '--repeat', '2',
           '--minibatch-steps', '6', '--no-extra-legs']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1, r.stdout[-2000:]
    out = json.loads(line[0])
    assert out['n_gpus'] == 2 and out['ranks_seen'] == [0, 1] and out['steps'] == 4 and out['scaling'] == 'strong'
    assert out['value'] > 0 and abs(out['value'] * out['ms_per_step'] / 1e3 - 1) < 0.01
    assert set(out['shard_modes_ms']) == {'single', 'split'} and out['shard_mode'] in out['shard_modes_ms']     # (300 samples per rank)
    assert out['collectives_per_step'] == {'single': 1, 'split': 2, 'buckets': 3}[out['shard_mode']]
    assert [p['rank'] for p in out['per_rank']] == [0, 1] and all(p['compute_ms'] > 0 and p['instances'] == 1 for p in out['per_rank'])
    assert out['scaling_model']['predicted_ms_per_step_no_overlap'] >= out['scaling_model']['shard_step_ms']
    assert len(out['repeat_ms_per_step']) == 2
    assert out['minibatch512']['steps'] == 6 and out['minibatch512']['value'] > 0
    assert out['roofline']['kernel'] in ('mesh_v2v_fused', 'gemm_pose_blend_bwd') and 0 < out['roofline']['frac'] < 1
    assert out['config']['parallelism'] == 'instance-shard x2'
    assert out['fallback'] == 'none' and [a['status'] for a in out['attempts']] == ['ok']
    assert all(c['agrees_with_single'] for c in out['shard_mode_check'].values())


@pytest.mark.gpu
def test_bench_two_ranks_fall_back_when_a_capture_kills_a_rank():
    """The driver's launch form with rank 1's worker dying inside its first sharded graph capture (fault injection in
    MultiViewModel._captured): the supervisors restart both workers with NEMO_GRAPH_COMM=0 and the line says so."""
    import socket
    if os.environ.get('NEMO_GRAPHS', '1') == '0':
        pytest.skip('NEMO_GRAPHS=0: nothing is captured, so nothing dies in a capture')
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, NEMO_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4',
               NEMO_TEST_FAIL_CAPTURE='exit')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), BENCH, '--gpus', '2', '--instances', '2', '--steps', '3', '--warmup', '1', '--repeat', '1',
           '--minibatch-steps', '0', '--no-extra-legs', '--shard-mode', 'single']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(line) == 1, r.stdout[-2000:]
    out = json.loads(line[0])
    assert out['n_gpus'] == 2 and out['value'] > 0
    assert out['fallback'] == 'NEMO_GRAPH_COMM=0' and out['graph_comm'] is False
    assert 'exit code 23' in out['attempts'][0]['status'] and out['attempts'][1]['status'] == 'ok'
