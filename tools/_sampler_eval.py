"""What the evaluation scripts share (inpaint_eval.py, solver_eval.py, adaptive_eval.py, posterior_eval.py, superres_eval.py,
guided_eval.py, adagn_eval.py, edm_eval.py, consistency_eval.py): the benchmark workload with a random-weight model on the
device, the timing of back-to-back launches (on one buffer set or rotating over several), of whole calls and of one network
evaluation, and the report."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import bench
import soft_truncation_amd as st


def parser(out_name):
  """--workload, --batch and --out (default profiles/<out_name>); the script adds its own."""
  ap = argparse.ArgumentParser()
  ap.add_argument('--workload', default='celebahq256', choices=sorted(bench.WORKLOADS))
  ap.add_argument('--batch', type=int, default=16)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', out_name))
  return ap


def workload(args):
  """(cfg_name, desc, cfg, device, sde, model, shape) of args.workload at args.batch: the model in eval mode, seed 0."""
  cfg_name, _, desc = bench.WORKLOADS[args.workload]
  cfg = st.configs.get_config(cfg_name)
  device = torch.device('cuda', 0)
  cfg.device = device
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  model = st.models.utils.create_model(cfg, sde)
  model.eval()
  return cfg_name, desc, cfg, device, sde, model, (args.batch, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)


def launches_alone(call, reps, bytes_moved):
  """(us per launch, TB/s of `bytes_moved`): `reps` back-to-back calls between two events, after 10 warm-ups."""
  for _ in range(10):
    call()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    call()
  e1.record()
  e1.synchronize()
  us = 1e3 * e0.elapsed_time(e1) / reps
  return us, bytes_moved / (us * 1e-6) / 1e12


ROTATE_BYTES, MAX_SETS = 1 << 30, 64


def set_count(per_set, most=MAX_SETS):
  """Buffer sets to rotate over so that ROTATE_BYTES pass between two uses of one set: at least 2, at most `most`."""
  sets = max(2, -(-ROTATE_BYTES // per_set))
  return sets if most is None else min(most, sets)


def rotating(call, sets):
  """A callable whose i-th call is ``call(sets[i % len(sets)])``."""
  state = {'i': 0}

  def step():
    call(sets[state['i'] % len(sets)])
    state['i'] += 1
  return step


def timed(calls, reps, warm=4):
  """us per call of `reps` calls between two events; call i is calls[i % len(calls)] (one per buffer set), after one warm-up
  of each of the first `warm` (None: all)."""
  for c in calls[:warm]:
    c()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for i in range(reps):
    calls[i % len(calls)]()
  e1.record()
  e1.synchronize()
  return 1e3 * e0.elapsed_time(e1) / reps


def wall(fn, rounds):
  """ms per call of each of the callables `fn` (a dict): wall time over a synchronisation, one warm-up each, `rounds`
  alternating rounds, medians."""
  for f in fn.values():
    f()
  torch.cuda.synchronize()
  took = {k: [] for k in fn}
  for r in range(rounds):
    for k in (list(fn) if r % 2 == 0 else reversed(list(fn))):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn[k]()
      torch.cuda.synchronize()
      took[k].append(1e3 * (time.perf_counter() - t0))
  return {k: statistics.median(v) for k, v in took.items()}


def evaluation(score_fn, sde, shape, device, reps=5):
  """ms of one ``score_fn(x, t)`` at t = 0.5 on a prior draw: wall time over a synchronisation, after 2 warm-ups."""
  x = sde.prior_sampling(shape).to(device)
  t = torch.ones(shape[0], device=device) * 0.5
  for _ in range(2):
    score_fn(x, t)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    score_fn(x, t)
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / reps


def write(lines, path):
  text = '\n'.join(lines)
  print(text)
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'w') as f:
    f.write(text + '\n')
