#!/usr/bin/env python
"""The DPM-Solver++ sampler (dpm_solver.py) on a benchmark workload: one launch of stk_dpm_update_f32
(include/stk_solver.h) on the sampler's state, timed alone and set against the 8 TB/s of HBM; one network evaluation; a
whole run of `--steps` steps with the final data prediction, in fp32 and in fp16 mode, and the largest difference between
the two results.  The recorded figures of the predictor-corrector sampler are quoted alongside.  The model has random
weights: the times do not depend on them, and sample quality is not measured here.  Writes profiles/dpm_solver_eval.txt.

    python tools/solver_eval.py --workload celebahq256 --batch 16 --steps 20
"""
import time

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = E.parser('dpm_solver_eval.txt')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--order', type=int, default=2)
ap.add_argument('--runs', type=int, default=2)
args = ap.parse_args()
_, desc, cfg, device, sde, model, shape = E.workload(args)
dpm, mutils = st.dpm_solver, st.models.utils
lib = dpm._library()
B, C, H, _ = shape
eps = 1e-3
schedule = dpm.dpm_schedule(sde, args.steps, order=args.order, eps=eps)
HBM_TBS = 8.0


def kernel_alone(second_order, n=200):
  """us per launch and TB/s of the bytes it moves: x and the score read, x written; second order also reads and writes the
  data prediction (20 B per element), first order neither (12 B)."""
  x, s = torch.randn(shape, device=device), torch.randn(shape, device=device)
  hist = torch.randn(shape, device=device) if second_order else None
  out = torch.empty_like(x)
  row = (1.3, 0.7, 0.45 if second_order else 0., 0.8, 0.35)
  bounds = dpm._clip_bounds(None)
  moved = 4 * x.numel() * (5 if second_order else 3)
  us, tbs = E.launches_alone(lambda: dpm._update(lib, x, s, hist, row, bounds, out, hist), n, moved)
  return us, moved, tbs


def evaluation():
  score_fn = mutils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  return E.evaluation(score_fn, sde, shape, device)


def whole_run(precision):
  sampler = dpm.get_dpm_sampler(cfg, sde, shape, st.datasets.get_data_inverse_scaler(cfg), steps=args.steps, order=args.order,
                                denoise=True, eps=eps, device=device, precision=precision)
  torch.manual_seed(1)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  x, nfe = sampler(model)
  torch.cuda.synchronize()
  assert bool(torch.isfinite(x).all())
  return time.perf_counter() - t0, nfe, x


lines = [f'{desc}, batch {B}: DPM-Solver++ order {args.order}, {args.steps} steps + the data prediction at eps = {eps}, logsnr '
         f'spacing; random weights; wall time over a device synchronisation, everything in one job on one box.']
with mutils.sampling_run(model):
  for name, second in (('second-order step (x, score, d_prev read; x, d written: 20 B per element)', True),
                       ('first-order step (x, score read; x written: 12 B per element)', False)):
    us, moved, tbs = kernel_alone(second)
    lines.append(f'stk_dpm_update_f32 alone on the [{B},{C},{H},{H}] state, {name}: {us:.1f} us per launch (200 back-to-back '
                 f'launches between two events), {moved / 1e6:.1f} MB = {tbs:.2f} TB/s = {100 * tbs / HBM_TBS:.0f} % of {HBM_TBS:.0f} TB/s')
  for precision in mutils.PRECISIONS:
    with mutils.precision(model, precision):
      lines.append(f'one network evaluation [{precision}]: {evaluation():.2f} ms')
results = {}
for precision in mutils.PRECISIONS:
  whole_run(precision)                                   # plans, arenas, prepared weights
  runs = [whole_run(precision) for _ in range(args.runs)]
  results[precision] = runs[-1][2]
  lines.append(f'whole run [{precision}], nfe = {runs[0][1]}: ' + ' / '.join(f'{r[0]:.3f}' for r in runs) + ' s')
diff = float((results['fp16'] - results['fp32']).abs().max())
lines.append(f'fp16 against fp32 result (same prior draw, after the inverse scaler): max |difference| {diff:.3e}, the fp32 result '
             f'lying in [{float(results["fp32"].min()):.3f}, {float(results["fp32"].max()):.3f}] (random weights: says nothing about '
             f'sample quality, which is unmeasured)')
lines.append('recorded for comparison (README, profiles/r06_sampler_eval_celebahq256.txt, profiles/fp16_sampler_eval.txt; NCSN++ 256^2, '
             'batch 16): predictor-corrector sampling 78.2 s at N = 1000, 156.6 s at N = 2000 (107.7 s in fp16 mode), 38.5 ms per '
             'network evaluation')
E.write(lines, args.out)
