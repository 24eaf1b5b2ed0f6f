#!/usr/bin/env python
"""The parallel-in-time sampler (parallel_sampling.py): what it costs.  (1) The three launches of include/stk_parallel.h on the
sampler's state, resident (one buffer set, back to back) and from HBM (rotating over buffer sets), beside their byte counts --
16 B per element and live slot for the scan (12 B at eta = 0), 8 B per element and slot for the slide at stride 1 (it is timed at
the fixed strides 1 and W / 2 and charged what it moves) -- and beside a torch
composition of the same iteration (cumsum, norms, roll).  (2) The ratio t(W B) / t(B) of one network evaluation for W in
{4, 16, 64}: DDPM++ 32x32 at B in {1, 16}, NCSN++ 256x256 at B = 1, one window at a time, with the memory the first evaluation
at each batch allocates (a window whose arena would not fit in the free memory is left out and said so).  (3) Whole runs against the window = 1 run of the same code.  Every comparison is the median of five alternating
rounds in one job on one box.  The model has random weights: the times do not depend on them, the iteration counts DO -- they
say nothing about a trained network -- and sample quality is not measured here.  Writes profiles/parallel_eval.txt.

    python tools/parallel_eval.py
"""
import gc
import statistics
import time

import torch

import _sampler_eval as E
from _sampler_eval import bench, st

ap = E.parser('parallel_eval.txt')
ap.add_argument('--steps', type=int, default=250, help='grid points of the whole runs')
ap.add_argument('--window', type=int, default=16)
ap.add_argument('--tol', type=float, default=0.01)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--skip-256', action='store_true', help='leave out the NCSN++ 256x256 evaluations')
ap.set_defaults(workload='cifar10', batch=16)
args = ap.parse_args()
ps, mutils, stk_lib = st.parallel_sampling, st.models.utils, st.engine.lib
lib = ps._library()
device = torch.device('cuda', 0)
HBM_TBS = 8.0
EPS = 1e-3


def load(name):
  cfg_name, _, desc = bench.WORKLOADS[name]
  cfg = st.configs.get_config(cfg_name)
  cfg.device = device
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  model = mutils.create_model(cfg, sde)
  model.eval()
  return desc, cfg, sde, model


def alternating(fns, rounds):
  """{name: median us per call}: each round times every entry of `fns` (name -> (calls, reps)) once, the order reversed every
  other round."""
  took = {k: [] for k in fns}
  for r in range(rounds):
    for k in (list(fns) if r % 2 == 0 else reversed(list(fns))):
      calls, reps = fns[k]
      took[k].append(E.timed(calls, reps, warm=None if r == 0 else 4))
  return {k: statistics.median(v) for k, v in took.items()}


# ---- (1) the launches ---------------------------------------------------------------------------------------------------
def launches(shape, W, noisy):
  """The scan and the stride on a full window (p = W); the slide at the fixed strides 1 and W / 2, read from buffers of
  their own that no timed launch writes (the stride launch writes a third).  Bytes are those the launch moves: the scan reads X,
  S (and Z) and writes Y per element and live slot; a slide by s reads the p - s slots that move and X[p] and writes all
  W + 1 slots -- 4 (2 W + 2 - s) B n, the 8 B per element and slot of the header at s = 1."""
  B, n = shape[0], shape[1] * shape[2] * shape[3]
  N = 4 * W
  ws_bytes = int(lib.picard_ws_bytes(W, B, n))
  per_set = 4 * B * n * (3 * W + 1)
  coef = (torch.rand(N, 3, device=device) * 0.1).contiguous()
  coef[:, 0].neg_()                                    # a - 1 < 0: repeated launches on one state stay bounded
  thr = torch.full((N,), 1e30, dtype=torch.float64, device=device)
  decided = torch.zeros(1, dtype=torch.int32, device=device)           # what the stride launch writes; nothing reads it
  slides = sorted({1, max(1, W // 2)})
  given = {s: torch.full((1,), s, dtype=torch.int32, device=device) for s in slides}
  stream = stk_lib.stream_ptr(device)

  def buffers():
    X = torch.randn(W + 1, B, n, device=device)
    S = torch.randn(W, B, n, device=device)
    Z = torch.randn(W, B, n, device=device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    return X, S, Z, ws

  def kernel_calls(bufs):
    X, S, Z, ws = bufs
    z = Z.data_ptr() if noisy else None
    calls = dict(
      scan=lambda: lib.picard_scan_f32(X.data_ptr(), S.data_ptr(), z, coef.data_ptr(), W, W, W, ws.data_ptr(), ws_bytes, B, n, stream),
      stride=lambda: lib.picard_stride(ws.data_ptr(), ws_bytes, thr.data_ptr(), W, W, W, B, n, decided.data_ptr(), None, stream))
    for s in slides:
      calls['slide', s] = (lambda s=s: lib.picard_slide_f32(X.data_ptr(), given[s].data_ptr(), W, W, B, n, stream))
    return calls

  def torch_iteration(bufs):
    X, S, Z, _ = bufs
    c = coef[W:2 * W]

    def call():
      D = c[:, 0, None, None] * X[:W] + c[:, 1, None, None] * S
      if noisy:
        D = D + c[:, 2, None, None] * Z
      Y = X[0] + torch.cumsum(D, dim=0)
      err = (Y[:-1] - X[1:W]).double().square().sum(dim=2)
      X[1:] = Y
      ok = (err <= thr[W + 1:2 * W, None]).all(dim=1)
      X.copy_(torch.roll(X, -1, dims=0))
      return ok
    return call

  sets = [buffers() for _ in range(E.set_count(per_set))]
  one = kernel_calls(sets[0])
  many = [kernel_calls(b) for b in sets]
  names = ['scan', 'stride'] + [('slide', s) for s in slides]
  fns = {}
  for name in names:
    fns[name, 'resident'] = ([one[name]], 200)
    fns[name, 'hbm'] = ([m[name] for m in many], 200)
  fns['torch', 'resident'] = ([torch_iteration(sets[0])], 50)
  fns['torch', 'hbm'] = ([torch_iteration(b) for b in sets], 50)
  us = alternating(fns, args.rounds)
  assert all(int(given[s]) == s for s in slides), 'a timed launch wrote the stride the slide reads'
  moved = {'scan': (16 if noisy else 12) * W * B * n, 'stride': ws_bytes}
  label = {'scan': 'stk_picard_scan_f32', 'stride': 'stk_picard_stride'}
  for s in slides:
    moved['slide', s] = 4 * (2 * W + 2 - s) * B * n
    label['slide', s] = f'stk_picard_slide_f32 at stride {s}'
  out = [f'the launches on X[{W + 1}, {B}, {n}] ({"with" if noisy else "without"} noise), p = W: one buffer set of {per_set / 1e6:.1f} MB '
         f'resident, or {len(sets)} sets in rotation ({len(sets) * per_set / 1e6:.0f} MB between two uses of a set); median of '
         f'{args.rounds} alternating rounds of 200 back-to-back launches; bytes are those the launch moves']
  for name in names:
    for where in ('resident', 'hbm'):
      t = us[name, where]
      rate = moved[name] / (t * 1e-6) / 1e12
      share = f' = {100 * rate / HBM_TBS:.0f} % of {HBM_TBS:.0f} TB/s' if where == 'hbm' and name != 'stride' else ''
      out.append(f'  {label[name]} {where}: {t:.1f} us, {moved[name] / 1e6:.2f} MB = {rate:.2f} TB/s{share}')
  for where in ('resident', 'hbm'):
    total = us['scan', where] + us['stride', where] + us[('slide', 1), where]
    out.append(f'  scan, stride and the slide at stride 1 together, {where}: {total:.1f} us; the torch composition (cumsum + norms + '
               f'roll by 1): {us["torch", where]:.1f} us')
  return out


# ---- (2) the evaluation at W B against B ------------------------------------------------------------------------------------
def release_programs(model):
  """Drop the engine's planned programs with their arenas: the next evaluation of a batch plans it again."""
  model.module.engine().programs.clear()
  gc.collect()
  torch.cuda.empty_cache()


def evaluation_ratios(desc, cfg, sde, model, B, windows):
  """One window at a time: only the programs of batch B and batch W B are alive, so the memory a first evaluation allocates
  is that batch's arena, and a large window is not refused for what the smaller ones hold.  A window whose arena, scaled up
  from the last one measured, would not fit in the free memory is left out and said so, not tried."""
  score_fn = mutils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  C, H = cfg.data.num_channels, cfg.data.image_size
  name = desc.split(',')[0]
  out, ratios, last = [], {}, None
  for W in windows:
    release_programs(model)
    free = torch.cuda.mem_get_info(device)[0]
    if last is not None:
      need = 1.1 * last[1] * W / last[0]
      if need > free:
        out.append(f'  {name}, B = {B}, W = {W}: not measured: by the arena at batch {last[0] * B} a batch of {W * B} needs about '
                   f'{need / 2 ** 30:.0f} GiB, {free / 2 ** 30:.0f} GiB are free')
        continue
    with mutils.sampling_run(model):
      calls, extra = {}, {}
      for reps in (1, W):
        x = sde.prior_sampling((reps * B, C, H, H)).to(device)
        t = torch.ones(reps * B, device=device) * 0.5
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        score_fn(x, t)
        torch.cuda.synchronize()
        extra[reps] = torch.cuda.memory_allocated() - before
        calls[reps] = (lambda x=x, t=t: score_fn(x, t))
      ms = E.wall(calls, args.rounds)
    last, ratios[W] = (W, extra[W]), ms[W] / ms[1]
    out.append(f'  {name}, B = {B}, W = {W}: t({W * B}) = {ms[W]:.2f} ms against t({B}) = {ms[1]:.2f} ms: ratio {ratios[W]:.2f} for '
               f'{W} x the work; the first evaluation at batch {W * B} allocated {extra[W] / 2 ** 20:.0f} MiB, at batch {B} '
               f'{extra[1] / 2 ** 20:.0f} MiB')
  release_programs(model)
  return out, ratios


# ---- (3) whole runs -------------------------------------------------------------------------------------------------------------
def whole_runs(desc, cfg, sde, model, shape, eta):
  inv = st.datasets.get_data_inverse_scaler(cfg)
  fns, samplers = {}, {}
  for W in (1, args.window):
    samplers[W] = ps.get_parallel_sampler(cfg, sde, shape, inv, steps=args.steps, window=W, tol=args.tol, eta=eta, denoise=True,
                                          eps=EPS, device=device)

    def run(W=W):
      torch.manual_seed(1)
      x, _ = samplers[W](model)
      assert bool(torch.isfinite(x).all())
    fns[W] = run
  ms = E.wall(fns, args.rounds)
  stats = samplers[args.window].last_stats
  return (f'  {desc.split(",")[0]}, batch {shape[0]}, {args.steps} steps, eta = {eta}, tol = {args.tol}: window 1 takes {ms[1] / 1e3:.2f} s '
          f'({args.steps} iterations); window {args.window} takes {ms[args.window] / 1e3:.2f} s in {stats["iterations"]} iterations, '
          f'{stats["evaluations"]} evaluations, largest stride {max(stats["strides"])} (random weights: the count says nothing '
          f'about a trained network)'), stats


t_start = time.perf_counter()
lines = ['The parallel-in-time sampler (parallel_sampling.py, include/stk_parallel.h) on an MI355X; random weights; everything in '
         'one job on one box.']
desc, cfg, sde, model = load(args.workload)
shape = (args.batch, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)
for noisy in (True, False):
  lines += launches(shape, args.window, noisy)
lines.append(f'one network evaluation at batch W B against batch B (wall time over a synchronisation, median of {args.rounds} '
             f'alternating rounds; one window at a time, the programs of the other batches released):')
ratios = {}
for B in (1, 16):
  got, ratios[B] = evaluation_ratios(desc, cfg, sde, model, B, (4, 16, 64))
  lines += got
runs = ['whole runs against the window = 1 run of the same code (the sequential sampler):']
for eta in (0., 1.):
  line, stats = whole_runs(desc, cfg, sde, model, shape, eta)
  runs.append(line)
  ratio = ratios.get(args.batch, {}).get(args.window)
  if ratio is not None:
    runs.append(f'    break-even N / (iterations x ratio) = {args.steps} / ({stats["iterations"]} x {ratio:.2f}) = '
                f'{args.steps / (stats["iterations"] * ratio):.2f} (above 1: the window run is the faster one)')
release_programs(model)
del model
gc.collect()
torch.cuda.empty_cache()
if not args.skip_256:
  desc, cfg, sde, model = load('celebahq256')
  lines += evaluation_ratios(desc, cfg, sde, model, 1, (4, 16, 64))[0]
lines += runs
lines.append(f'this report took {time.perf_counter() - t_start:.0f} s')
E.write(lines, args.out)
