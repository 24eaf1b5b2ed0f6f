#!/usr/bin/env python
"""The data-consistency launch of the super-resolution sampler, stk_superres_f32 (include/stk_superres.h), timed alone on a
[batch,3,size,size] state for each factor, against the same step composed from torch operations (avg_pool2d, two
repeat_interleave per output and the element-wise passes between them) on the same box, and against its own byte count:
x read once, x and x_mean written once, low and z read (3 + 2/P state-sized tensors, P = factor^2).

The state is 12.6 MB at 256^2, batch 16, so three of them stay in the 256 MiB last-level cache between launches; every figure
is therefore taken twice, on one set of buffers (cache-resident) and rotating over enough sets to exceed the cache (from
HBM).  Launches run back to back between two device events after warm-ups; the two forms alternate, three rounds, all
rounds printed.  Writes profiles/superres_eval.txt.  Sample quality is not measured here or anywhere else.

    python tools/superres_eval.py --batch 16 --size 256
"""
import argparse
import os

import torch
import torch.nn.functional as F

import _sampler_eval as E
from _sampler_eval import st

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--reps', type=int, default=2000)
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'superres_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'superres_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
cg = st.controllable_generation
lib = cg._superres_library()
B, C, H = args.batch, 3, args.size
CACHE = 256 << 20


def buffers(r):
  x = torch.randn(B, C, H, H, device=device)
  low, z = torch.randn(B, C, H // r, H // r, device=device), torch.randn(B, C, H // r, H // r, device=device)
  return x, low, z, torch.empty_like(x), torch.empty_like(x)


def composed(x, low, z, a, s, r):
  """The launch as torch operations -> (x, x_mean)."""
  wide = lambda v: v[:, None, None, None]
  up = lambda v: v.repeat_interleave(r, dim=2).repeat_interleave(r, dim=3)
  m = F.avg_pool2d(x, r)
  mean = wide(a) * low
  known = mean + wide(s / r) * z
  return x + up(known - m), x + up(mean - m)


lines = [f'stk_superres_f32 on a [{B},{C},{H},{H}] fp32 state, x_mean written, {args.reps} back-to-back launches between two device '
         f'events after 10 warm-ups; three rounds, kernel and torch composition alternating.  "resident": one set of buffers (it '
         f'fits the 256 MiB last-level cache); "rotating": as many sets as exceed that cache.']
a = torch.rand(B, device=device) + 0.25
s = torch.rand(B, device=device) + 0.05
for r in cg.FACTORS:
  moved = 4 * (3 * B * C * H * H + 2 * B * C * (H // r) ** 2)
  n_sets = CACHE // moved + 2
  sets = [buffers(r) for _ in range(n_sets)]
  kernel = lambda x, low, z, out, mean: cg._superres(lib, x, low, z, a, s, r, out, mean)
  torch_form = lambda x, low, z, out, mean: composed(x, low, z, a, s, r)
  # the two forms agree on what they compute (the restatement in float64 is the tests' business)
  kernel(*sets[0])
  want = composed(*sets[0][:3], a, s, r)
  assert float((sets[0][3] - want[0]).abs().max()) < 1e-4 and float((sets[0][4] - want[1]).abs().max()) < 1e-4
  rounds = []
  for _ in range(3):
    rounds.append((E.launches_alone(lambda: kernel(*sets[0]), args.reps, moved),
                   E.launches_alone(lambda: torch_form(*sets[0]), args.reps, moved),
                   E.launches_alone(E.rotating(lambda b: kernel(*b), sets), args.reps, moved),
                   E.launches_alone(E.rotating(lambda b: torch_form(*b), sets), args.reps, moved)))
  lines.append(f'factor {r}: {moved / 1e6:.1f} MB per launch by its byte count, {n_sets} buffer sets when rotating')
  for j, name in enumerate(('kernel, resident', 'torch,  resident', 'kernel, rotating', 'torch,  rotating')):
    best = min(rd[j][0] for rd in rounds)
    lines.append(f'  {name}: ' + ' / '.join(f'{rd[j][0]:.1f}' for rd in rounds) + f' us per step; fastest {best:.1f} us = '
                 f'{moved / (best * 1e-6) / 1e12:.2f} TB/s of the kernel\'s byte count')
  k_res, t_res, k_rot, t_rot = (min(rd[j][0] for rd in rounds) for j in range(4))
  lines.append(f'  torch composition / kernel: {t_res / k_res:.1f}x resident, {t_rot / k_rot:.1f}x rotating')
  del sets
lines.append('Sample quality of the super-resolution sampler is unmeasured.')
E.write(lines, args.out)
