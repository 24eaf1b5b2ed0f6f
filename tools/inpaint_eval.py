#!/usr/bin/env python
"""One iteration of the inpainting sampler against one iteration of the plain PC sampler: the same model, batch, box and
update rules (reverse diffusion + Langevin, one corrector step), weights prepared once, forward only.  An iteration is the
corrector update and the predictor update (two network evaluations); the inpainting iteration adds to each the per-image
coefficients of sde.marginal_prob, one randn_like and one launch of stk_impute_f32 (include/stk_impute.h).  The launch is
also timed alone, with and without the colour mix.  Writes profiles/controllable_eval.txt.

    python tools/inpaint_eval.py --workload celebahq256 --batch 16 --iters 10
"""
import time

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = E.parser('controllable_eval.txt')
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--precision', default='fp32', choices=('fp32', 'fp16'))
args = ap.parse_args()
_, desc, cfg, device, sde, model, (B, C, H, _) = E.workload(args)
cg, S = st.controllable_generation, st.sampling
lib = cg._library()
predict, correct = S.pc_updates(cfg, sde, S.get_predictor('reverse_diffusion'), S.get_corrector('langevin'), cfg.sampling.snr, 1,
                                False, cfg.training.continuous)
data = torch.rand(B, C, H, H, device=device)
mask = torch.zeros(1, 1, H, H, device=device)
mask[..., : H // 2, :] = 1.
form = cg.mask_form(mask, data)
t = torch.tensor(0.5)


def plain(x):
  vec_t = torch.ones(B, device=device) * t
  x, _ = correct(x, vec_t, model=model)
  return predict(x, vec_t, model=model)[0]


def inpaint(x):
  x, _ = cg._half_step(lib, correct, sde, model, data, mask, form, x, t, None)
  return cg._half_step(lib, predict, sde, model, data, mask, form, x, t, None)[0]


def timed(step, n):
  x = torch.randn(B, C, H, H, device=device)
  for _ in range(3):
    x = step(x)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(n):
    x = step(x)
  torch.cuda.synchronize()
  assert bool(torch.isfinite(x).all())
  return 1e3 * (time.perf_counter() - t0) / n


def kernel_alone(mix, n=200):
  x, z = torch.randn(B, C, H, H, device=device), torch.randn(B, C, H, H, device=device)
  out, mean = torch.empty_like(x), torch.empty_like(x)
  a = s = torch.ones(B, device=device)
  m, f = (cg.get_mask(x[:1]), (1, 3)) if mix else (mask, form)
  moved = 4 * (5 * x.numel() + m.numel())            # x, data, z read, x and x_mean written, the mask read once
  return E.launches_alone(lambda: cg._impute(lib, x, data, z, m, f, a, s, out, mean, mix), n, moved)


lines = [f'{desc} [{args.precision}], batch {B}: reverse diffusion + Langevin (1 step), t = 0.5, {args.iters} iterations after 3 '
         f'warm-ups, weights prepared once; wall time over a device synchronisation, modes alternated in one job on one box.']
with st.models.utils.sampling_run(model, args.precision):
  runs = [(timed(plain, args.iters), timed(inpaint, args.iters)) for _ in range(2)]
  alone = [(name, kernel_alone(mix)) for name, mix in (('inpainting (no colour mix)', None), ('colourisation (3x3 mix)', cg._MIX_BLEND))]
p, i = min(r[0] for r in runs), min(r[1] for r in runs)
lines.append('  plain PC iteration (2 network evaluations):      ' + ' / '.join(f'{r[0]:.3f}' for r in runs) + ' ms')
lines.append('  inpainting iteration (the same + 2 imputations): ' + ' / '.join(f'{r[1]:.3f}' for r in runs) + ' ms')
lines.append(f'  difference of the faster runs: {i - p:+.3f} ms per iteration = {100 * (i - p) / p:+.2f} % of the plain iteration')
lines.append(f'stk_impute_f32 alone on the [{B},{C},{H},{H}] state (200 back-to-back launches between two events, x_mean written, a '
             f'[1,1,H,W] / [1,3,H,W] mask):')
for name, (us, tbs) in alone:
  lines.append(f'  {name}: {us:.1f} us per launch, {tbs:.2f} TB/s of the 20 B per element it moves')
E.write(lines, args.out)
