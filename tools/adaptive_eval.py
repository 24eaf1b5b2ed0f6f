#!/usr/bin/env python
"""The adaptive-step SDE sampler (adaptive_sde.py) on a benchmark workload: the three launches of include/stk_adaptive.h on
the sampler's state, timed alone and set against the 8 TB/s of HBM; whole runs at rtol 0.01 and 0.05 (iterations, share of
rejected sample-steps, wall time); and the predictor-corrector sampler at N = `--pc-steps` in the same job on the same box.
The model has random weights: the times per launch and per evaluation do not depend on them, the iteration counts DO (a
trained score is smoother), and sample quality is not measured here.  Writes profiles/adaptive_eval.txt.

    python tools/adaptive_eval.py --workload celebahq256 --batch 16
"""
import time

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = E.parser('adaptive_eval.txt')
ap.add_argument('--rtols', type=float, nargs='+', default=[0.01, 0.05])
ap.add_argument('--pc-steps', type=int, default=1000, help='N of the predictor-corrector run (0: skip it)')
args = ap.parse_args()
cfg_name, desc, cfg, device, sde, model, shape = E.workload(args)
ada, mutils, stk_lib = st.adaptive_sde, st.models.utils, st.engine.lib
lib = ada._library()
B, C, H, _ = shape
n = C * H * H
eps = 1e-3
atol = ada.default_atol(cfg)
HBM_TBS = 8.0


def launches_alone(reps=200):
  """us per launch of each entry on the state, and the bytes it moves: stage reads x, score, z and writes x1 (4 tensors);
  heun_error reads x, x1, x1_prev, score2, z and writes x2 (6); commit reads x2, x1 and writes x, x1_prev where accepted (4,
  every sample accepted here)."""
  x, s, z, x1, x1_prev, x2 = (torch.randn(shape, device=device) for _ in range(6))
  xc, pc = x.clone(), x1_prev.clone()
  t, h = torch.full((B,), 0.5, device=device), torch.full((B,), 0.01, device=device)
  row1, row2 = ada.stage_rows(sde, t, h), ada.heun_rows(sde, ada.next_time(t, h, eps), h)
  ws_bytes = lib.sde_ws_bytes(B, n)
  ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
  t_out, h_out, err = (torch.empty(B, device=device) for _ in range(3))
  accept = torch.empty(B, dtype=torch.int32, device=device)
  stream = stk_lib.stream_ptr(device)
  p = lambda v: v.data_ptr()
  calls = {
    'stk_sde_stage_f32': (4, lambda: lib.sde_stage_f32(p(x), None, p(s), p(z), p(row1), p(x1), B, n, stream)),
    # rtol = 1e30: every sample is accepted, so commit moves all it can
    'stk_sde_heun_error_f32': (6, lambda: lib.sde_heun_error_f32(p(x), p(x1), p(x1_prev), p(s), p(z), p(row2), atol, 1e30, p(x2),
                                                                 p(ws), ws_bytes, B, n, stream)),
    'stk_sde_commit_f32': (4, lambda: lib.sde_commit_f32(p(xc), p(pc), p(x2), p(x1), p(t), p(h), eps, 0.9, 0.9, p(ws), ws_bytes,
                                                         p(t_out), p(h_out), p(err), p(accept), B, n, stream)),
  }
  out = []
  for name, (tensors, call) in calls.items():
    moved = 4 * x.numel() * tensors
    us, tbs = E.launches_alone(call, reps, moved)
    out.append((name, us, moved, tbs))
  assert int(accept.sum()) == B
  return out


def evaluation():
  score_fn = mutils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  return E.evaluation(score_fn, sde, shape, device)


def adaptive_run(rtol):
  with mutils.sampling_run(model):
    score_fn = mutils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
    torch.manual_seed(1)
    x = sde.prior_sampling(shape).to(device).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, iterations, info = ada.adaptive_sample(score_fn, x, sde, rtol=rtol, atol=atol, eps=eps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
  accepted, rejected = int(info['accepted'].sum()), int(info['rejected'].sum())
  assert bool(torch.isfinite(x).all())
  return wall, iterations, rejected / max(1, accepted + rejected)


def pc_run(N):
  c = st.configs.get_config(cfg_name)
  c.device = device
  c.model.num_scales = N
  c.sampling.method = 'pc'
  sde_n = st.sde_lib.get_sde(c, None)
  fn = st.sampling.get_sampling_fn(c, sde_n, shape, st.datasets.get_data_inverse_scaler(c), eps)
  torch.manual_seed(1)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  _, nfe = fn(model)
  torch.cuda.synchronize()
  return time.perf_counter() - t0, nfe


lines = [f'{desc}, batch {B}: adaptive-step SDE sampler, atol {atol}, h_init 0.01, safety 0.9, exponent 0.9, eps = {eps}; random '
         f'weights; wall time over a device synchronisation, everything in one job on one box.']
with mutils.sampling_run(model):
  total = 0.
  for name, us, moved, tbs in launches_alone():
    total += us
    lines.append(f'{name} alone on the [{B},{C},{H},{H}] state: {us:.1f} us per launch (200 back-to-back launches between two '
                 f'events), {moved / 1e6:.1f} MB = {tbs:.2f} TB/s = {100 * tbs / HBM_TBS:.0f} % of {HBM_TBS:.0f} TB/s')
  lines.append(f'the three launches of one iteration together: {total:.1f} us')
  lines.append(f'one network evaluation [fp32]: {evaluation():.2f} ms')
for rtol in args.rtols:
  wall, iterations, share = adaptive_run(rtol)
  lines.append(f'whole run at rtol {rtol}: {iterations} iterations (nfe = {2 * iterations}), {100 * share:.1f} % of the sample-steps '
               f'rejected, {wall:.2f} s')
if args.pc_steps:
  wall, nfe = pc_run(args.pc_steps)
  lines.append(f'predictor-corrector sampler at N = {args.pc_steps} in the same job: nfe = {nfe}, {wall:.2f} s')
E.write(lines, args.out)
