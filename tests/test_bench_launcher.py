"""`python bench.py --gpus N` must itself bring up N ranks when it is not already under a launcher (the round-1
bench parsed the flag and ran one process).  CPU check of that plumbing: --launch-check stops after the process
group is up (gloo here, RCCL on a GPU node) and the ranks are counted with one all-reduce."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_gpus_2_launches_two_ranks():
  env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--launch-check'],
                       capture_output=True, text=True, env=env, timeout=280)
  assert out.returncode == 0, out.stderr[-2000:]
  lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, out.stdout
  rec = json.loads(lines[0])
  assert rec['n_gpus'] == 2 and rec['ranks_counted'] == 2 and rec['launch_check'] is True


def test_bench_single_process_stays_single():
  env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--launch-check'],
                       capture_output=True, text=True, env=env, timeout=120)
  assert out.returncode == 0, out.stderr[-2000:]
  rec = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][0])
  assert rec['n_gpus'] == 1 and rec['ranks_counted'] == 1


def _bench_ranks(tmp_path, ranks=2, **env_extra):
  """tests/_bench_worker.py as ranks 0 .. ranks - 1 over gloo (ranks = 1: one process, no group); returns their (stdout,
  stderr) after checking every rank exited 0."""
  import socket
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'oracle')])
  base = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
  base.update(WORLD_SIZE=str(ranks), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), BENCH_DETAIL=str(tmp_path / 'detail.json'),
              STK_POISON='1', **env_extra)
  procs = []
  for rank in range(ranks):
    env = dict(base, RANK=str(rank), LOCAL_RANK=str(rank))
    procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', '_bench_worker.py')], env=env,
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
  outs = [p.communicate(timeout=560) for p in procs]
  for p, (so, se) in zip(procs, outs):
    assert p.returncode == 0, se[-3000:]
  return outs


@pytest.mark.timeout(600)
def test_bench_main_two_ranks_emits_one_short_line(tmp_path):
  """bench.py's real main() at WORLD_SIZE = 2 through to the emitted stdout line, on the CPU checker over gloo
  (tests/_bench_worker.py replaces four seams only): n_gpus = 2, value = GLOBAL images/s, the line is short and alone."""
  outs = _bench_ranks(tmp_path, BENCH_FULL='1')
  assert outs[1][0] == '', outs[1][0]                       # only rank 0 writes to stdout
  stdout0 = outs[0][0]
  assert stdout0.count('\n') == 1 and len(stdout0) < 4000, stdout0
  line = json.loads(stdout0)
  assert line['n_gpus'] == 2 and line['config']['parallelism'] == 'dp2'
  assert line['config']['per_gpu_batch'] == 4 and line['config']['global_batch'] == 8
  assert line['steps'] == 3 and line['warmup'] == 1 and line['scaling'] == 'weak' and line['unit'] == 'images/s'
  # value is the whole job's rate: global batch x steps / max-over-ranks elapsed
  assert line['value'] == pytest.approx(8 * 1e3 / line['ms_per_step'], rel=1e-3)
  # --full, no GPU here: the exchange-stream probe cannot run, and the line says so instead of staying silent
  assert line['exchange_serialised'] is True and 'error' in line['exchange_stream']
  detail = json.load(open(line['detail']))
  assert detail['n_gpus'] == 2 and detail['value'] == pytest.approx(line['value'], rel=1e-3)
  assert len(outs[0][1]) < 4000, outs[0][1][-4000:]         # stderr stays short too (no progress bars, no tables)


@pytest.mark.timeout(900)
def test_bench_dump_outputs_is_repeatable(tmp_path):
  """--dump-outputs DIR: the last timed step's losses and a fixed sample of the parameters and EMA it left, as float32 .npy
  files, identical from run to run with the same arguments; --steps sets the timed steps and the line reports ms_per_step."""
  import numpy as np
  dumps = []
  for run in range(2):
    d = tmp_path / f'dump{run}'
    outs = _bench_ranks(tmp_path, BENCH_STEPS='2', BENCH_DUMP=str(d))
    line = json.loads(outs[0][0])
    assert line['steps'] == 2 and line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(8 * 1e3 / line['ms_per_step'], rel=1e-3)
    dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
  a, b = dumps
  assert set(a) == {'losses.npy', 'params.npy', 'ema.npy'}
  assert sum(v.nbytes for v in a.values()) <= 64 << 20
  assert a['losses.npy'].shape == (4,)                       # rank 0's per-GPU batch
  for name, v in a.items():
    assert v.dtype == np.float32 and np.isfinite(v).all(), name
    assert np.array_equal(v, b[name]), name
  assert not np.array_equal(a['params.npy'], a['ema.npy'])   # the EMA trails the weights


@pytest.mark.timeout(600)
def test_plain_run_measures_only_the_headline(tmp_path):
  """Without --full, bench.py's real main() sets up, warms up, times the steps, dumps and prints the line -- nothing else: no
  exchange-stream probe at N = 2; at N = 1 no exchange proxy, arithmetic check, library-GEMM probe, sampler, CPU baseline,
  parity probe or other workloads; no per-kernel event brackets (--no-kernel-timer is not given: they are --full's too)."""
  extras = ('exchange_stream', 'exchange_proxy', 'roofline', 'roofline_best', 'kernels', 'arithmetic_check', 'pipe_probe_error',
            'sampler', 'cpu_baseline', 'parity_probe', 'workloads')
  for ranks in (2, 1):
    outs = _bench_ranks(tmp_path, ranks=ranks, BENCH_DUMP=str(tmp_path / f'dump{ranks}'), BENCH_KERNEL_TIMER='1')
    line = json.loads(outs[0][0])
    detail = json.load(open(line['detail']))
    assert line['n_gpus'] == ranks and line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(4 * ranks * 1e3 / line['ms_per_step'], rel=1e-3)
    assert set(line['headline']) == {'cifar10'} and 'step_roofline' in line
    for k in extras:
      assert k not in line and k not in detail, (ranks, k)
    assert 'exchange_serialised' not in line
    assert sorted(os.listdir(tmp_path / f'dump{ranks}')) == ['ema.npy', 'losses.npy', 'params.npy']
