"""The DMA ring of the plane-operand 3x3 weight gradient (csrc/conv_x2w.h, x2w::wgrad_kernel) against float64.

The kernel prefetches chunk c + 1 into one LDS stage while its MFMAs read chunk c from the other, and only its own wait and
barrier at the loop head order the two.  A stage read early or refilled late is data of a NEIGHBOURING chunk, so every image
here has its own offset and scale in both operands: the wrong chunk cannot add up to the right sum.  `wgs` chooses the K
split (x2w::plan keeps >= 8 chunks per workgroup), which sets where a workgroup's chunks start and end: in mid-image, across
image boundaries, one workgroup for everything; both group forms on the 16- and 8-wide maps, odd round counts (the second
group idles in the last round), dead waves (Cout % 128 != 0), the 8- and 4-wide maps, and W > 32 where the dy tile's halo
columns are pixels and keep their own DMA (on the 32- and 16-wide maps they are zeroed once in front of the loop).

Bound: PL_WGRAD_RTOL relative to max|alpha sum dy x|, as tests/test_planes.py::test_wgrad_from_planes applies it, against a
float64 reference computed here.  Each case runs three times into a NaN-filled workspace; the three results are bit-equal.
"""
import pytest
import torch

from _tolerances import PL_WGRAD_RTOL
from _util import call, dev_of, rnd

pytestmark = pytest.mark.gpu

CASES = [
  # (N, Cin, Cout, H), wgs (0: the default of a launch beside another stream)
  ((3, 64, 128, 32), 16),     # 12-row splits that start in mid-image and cross the image boundaries
  ((3, 64, 128, 32), 48),     # the deepest split the plan allows (8 rows)
  ((1, 32, 32, 32), 1),       # one workgroup walks the whole image
  ((1, 32, 32, 32), 4),
  ((8, 32, 128, 16), 0),      # two groups, 8 rounds each
  ((8, 32, 128, 16), 3),      # odd split count: one group
  ((8, 32, 128, 16), 6),      # two groups, 11 rounds; the last split is shorter
  ((3, 96, 96, 16), 0),       # one group, a dead wave (three 32-channel blocks of dy)
  ((3, 96, 96, 16), 6),       # two groups, a dead wave in each
  ((8, 64, 160, 8), 0),       # 8-wide maps, two groups, ragged second co tile
  ((8, 64, 160, 8), 4),       # ... one group
  ((18, 64, 160, 4), 0),      # 4-wide maps: a chunk is two images, 9 rounds
  ((2, 32, 32, 64), 0),       # W > 32: a chunk is half a row
  ((2, 32, 32, 64), 3),
  ((1, 32, 64, 128), 0),      # W = 128: four chunks per row
  ((1, 32, 64, 128), 5),      # 103 chunks per split: splits start in mid-row
]

_ref_cache = {}


def _per_image(N, seed):
  """a different offset and scale for every image"""
  g = torch.Generator().manual_seed(seed)
  off = torch.linspace(-1.0, 1.0, N)[torch.randperm(N, generator=g)] if N > 1 else torch.tensor([0.5])
  scale = torch.logspace(-1, 0, N)[torch.randperm(N, generator=g)] if N > 1 else torch.tensor([1.0])
  return off[:, None, None, None], scale[:, None, None, None]


def _operands(shape):
  """x, dy, dw0 and the float64 weight gradient of one shape (computed once, shared by the shape's cases, never modified)"""
  if shape not in _ref_cache:
    N, Cin, Cout, H = shape
    ox, sx = _per_image(N, 11)
    oy, sy = _per_image(N, 12)
    x = (rnd(N, Cin, H, H, seed=1) * sx + ox).contiguous()
    dy = (rnd(N, Cout, H, H, seed=2) * sy + oy).contiguous()
    dw0 = rnd(Cout, Cin, 3, 3, seed=3)
    g = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), dy.double(), padding=1)
    _ref_cache[shape] = (x, dy, dw0, g)
  return _ref_cache[shape]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d_%dto%d_%dx%d_wgs%d' % (*c[0], c[0][3], c[1]))
def test_wgrad_ring_against_float64(hip_lib, case):
  shape, wgs = case
  N, Cin, Cout, H = shape
  lib = hip_lib
  assert int(lib.conv2d_wgrad_pl_ok(N, H, H, Cin, Cout)) == 1
  x, dy, dw0, g = _operands(shape)
  alpha = 0.5
  d = dev_of(lib)
  xd, dyd = x.to(d), dy.to(d)
  ax, ay = torch.zeros(256, device=d), torch.zeros(256, device=d)
  call(lib, 'amax_partial_f32', xd, xd.numel(), ax)
  call(lib, 'amax_partial_f32', dyd, dyd.numel(), ay)
  xp = torch.zeros(int(lib.planes_bytes(N, Cin, H * H)), dtype=torch.uint8, device=d)
  yp = torch.zeros(int(lib.planes_bytes(N, Cout, H * H)), dtype=torch.uint8, device=d)
  call(lib, 'split_planes_f32', xd, N, Cin, H * H, ax, 256, xp)
  call(lib, 'split_planes_f32', dyd, N, Cout, H * H, ay, 256, yp)
  nb = int(lib.conv2d_wgrad_pl_ws_bytes(N, H, H, Cin, Cout))
  outs = []
  for _ in range(3):
    ws = torch.full((nb // 4 + 64,), float('nan'), device=d)
    dw = dw0.clone().to(d)
    call(lib, 'conv2d_wgrad_pl_wgs_f32', xp, ax, yp, ay, dw, alpha, ws, nb, N, H, H, Cin, Cout, wgs)
    outs.append(dw.cpu())
  scale = (alpha * g).abs().max().item()
  err = (outs[0].double() - (dw0.double() + alpha * g)).abs().max().item()
  print(f'  wgrad ring {shape} wgs {wgs}: max|err| / max|alpha sum dy x| = {err / scale:.3e}  (bound {PL_WGRAD_RTOL:.0e})')
  assert torch.isfinite(outs[0]).all()
  assert err <= PL_WGRAD_RTOL * scale
  for i in (1, 2):
    assert torch.equal(outs[i], outs[0]), f'run {i} differs from run 0'
