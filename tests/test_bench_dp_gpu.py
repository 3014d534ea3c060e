"""Rehearsal of bench.py's N>1 path on ONE card: two ranks under torch.distributed.run share cuda:0 and exchange
gradients through gloo (MCGEN_DIST_BACKEND=gloo; RCCL refuses two ranks on one device).  Checks the launch
contract (env rendezvous on 127.0.0.1, graph capture with a live process group, all-reduce between replays,
max-over-ranks timing, the collective-free roofline pass on rank 0 while the other rank waits at the final barrier,
one JSON line from rank 0) -- not performance."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('workload,batch,extra', [('mcpixelcnn', 16, []), ('cifar10', 16, []),
                                                  # BASELINE configs[2]'s per-GPU shard (global 512 over 8 GPUs = 64 / GPU), bf16 gradient wire
                                                  ('coil100', 64, ['--grad-bf16'])])
def test_bench_two_ranks_one_card(workload, batch, extra):
    env = dict(os.environ, MCGEN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29533', os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--workload', workload, '--steps', '2',
           '--warmup', '1', '--batch', str(batch), '--full', '--sustain-steps', '0'] + extra
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 2 and out['scaling'] == 'weak'
    assert out['config']['global_batch'] == 2 * batch and out['value'] > 0
    if workload in ('cifar10', 'coil100'):
        # N > 1 line: the gradient exchange's own time per iteration and the part of it hidden under the backward pass
        assert out['comm'] is not None and out['comm']['comm_us'] > 0
        assert 0 <= out['overlap_us'] <= out['comm']['comm_us'] + 1e-6 and out['grad_wire_dtype'] == ('bf16' if extra else 'f32')


@pytest.mark.parametrize('workload', ['cifar10', 'coil100'])
def test_bench_default_path_replays_graphs(workload):
    """The single-GPU bench command at its real batch: the HIP-graph capture must succeed (an eager fall-back would still
    print a line -- `config.graph_replay` says which path was timed) and the line carries the contract's keys."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', workload, '--steps', '3', '--warmup', '1',
           '--full', '--no-cpu-baseline', '--sustain-steps', '0']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert out['config']['graph_replay'] is True, r.stderr[-3000:]
    assert out['n_gpus'] == 1 and out['value'] > 0 and out['mask_compaction'] is True
    rf = out['roofline']
    assert rf['unit'] in ('TFLOP/s', 'GB/s') and 0 < rf['frac'] < 1 and rf['bound'] in ('mfma', 'hbm')


def test_bench_plain_run_is_headline_only():
    """Without --full the line carries the headline figure and nothing that needs runs of its own: no sustained loop, no
    roofline pass, no CPU baseline; the iterations it ran are the warm-up and the timed steps."""
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert out['metric'] == 'images/sec (train step) MCGAN CIFAR-10 32x32' and out['unit'] == 'images/s'
    assert out['higher_is_better'] is True and out['dtype'] == 'bf16' and out['steps'] == 3 and out['warmup'] == 1
    assert out['value'] > 0 and abs(out['value'] * out['ms_per_step'] - 128 * 1e3) < 1e-6 * 128 * 1e3
    assert out['config']['graph_replay'] is True, r.stderr[-3000:]
    assert out['roofline'] is None and out['cpu_baseline'] is None and out['comm'] is None
    assert out['sustained_ms_per_step'] is None and out['sustain_steps'] == 0 and out['loss_trace']['iterations'] == 4


def test_bench_dump_outputs_last_timed_step(tmp_path):
    """--dump-outputs DIR: the losses of the last timed step (the JSON line's last_losses) and the state_dict it left in the
    model, as .npy files; the same arguments give the same files."""
    import numpy as np
    outs = []
    for d in ('a', 'b'):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--no-cpu-baseline',
               '--sustain-steps', '0', '--no-roofline', '--dump-outputs', str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1]))
    assert outs[0]['steps'] == 2
    files = sorted(os.listdir(tmp_path / 'a'))
    assert 'state.generator.linear.module.weight.npy' in files and sorted(os.listdir(tmp_path / 'b')) == files
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64_000_000
    got = (float(np.load(tmp_path / 'a' / 'd_loss.npy')), float(np.load(tmp_path / 'a' / 'g_loss.npy')))
    assert got == tuple(outs[0]['last_losses'])
    for f in files:
        x = np.load(tmp_path / 'a' / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, np.load(tmp_path / 'b' / f)), f
