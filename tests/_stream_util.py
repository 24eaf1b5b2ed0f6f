"""Helpers of the GPU tests of the streaming kernels (test_gpu_impute.py, test_gpu_dpm_solver.py, test_gpu_adaptive_sde.py
and the files since):
operands on the 16-byte and on the scalar path, and the per-element rounding bound k u B."""
import numpy as np
import torch

U = 2.0 ** -24


def shifted(t, dev):
  """A contiguous copy of t that starts 4 bytes into its buffer: a view no 16-byte access may touch."""
  buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
  view = buf[1:].view(t.shape)
  view.copy_(t)
  assert view.is_contiguous() and view.data_ptr() % 16 == 4
  return view


def place(t, dev, one_in=False):
  """A fresh copy of t (a tensor or a numpy array) on dev: aligned, or entered one element into its buffer."""
  if isinstance(t, np.ndarray):
    t = torch.from_numpy(np.ascontiguousarray(t))
  return shifted(t, dev) if one_in else t.to(dev).clone()


def within(got, want, mag, k, what, show=False):
  """|got - want| <= k u B, element by element, u = 2^-24; want and B = mag are float64, tensors or numpy arrays.  Returns
  the worst ratio err / (u B), and prints it with show."""
  want, mag = torch.as_tensor(want), torch.as_tensor(mag)
  err = (got.detach().cpu().double() - want).abs()
  assert torch.isfinite(err).all(), f'{what}: non-finite result'
  units = float((err / (U * mag).clamp_min(1e-300)).max())
  if show:
    print(f'{what}: worst error {units:.2f} x 2^-24 B (bound {k})')
  assert bool((err <= k * U * mag).all()), f'{what}: {units:.2f} x 2^-24 B exceeds {k}'
  return units


GUARD = 8                      # sentinel elements before and after a guarded view
SENTINEL = {torch.float32: -1.5 * 2.0 ** 79, torch.float64: -1.5 * 2.0 ** 79, torch.float16: -1234.0, torch.uint8: 0xA5}
ENTERED = {'aligned': 0, 'entered-one-in': 1, 'entered-two-in': 2}


class Guarded:
  """A fresh copy of t (a tensor or a numpy array) on dev with GUARD sentinel elements before and after it (bytes for a
  uint8 tensor), placed 'aligned' (data_ptr % 16 == 0), 'entered-one-in' (% 16 == 4) or 'entered-two-in' (% 16 == 8; the
  entered placements are float32's).  .view is the operand; .check() asserts that no sentinel was written."""

  def __init__(self, t, dev, placement='aligned'):
    if isinstance(t, np.ndarray):
      t = torch.from_numpy(np.ascontiguousarray(t))
    entered = ENTERED[placement]
    assert entered == 0 or t.dtype == torch.float32, (placement, t.dtype)
    self.lead, self.n = GUARD + entered, t.numel()
    self.buf = torch.full((self.lead + self.n + GUARD,), SENTINEL[t.dtype], dtype=t.dtype, device=dev)
    self.view = self.buf[self.lead:self.lead + self.n].view(t.shape)
    self.view.copy_(t)
    assert self.view.is_contiguous() and self.buf.data_ptr() % 16 == 0
    if t.dtype == torch.float32:
      assert self.view.data_ptr() % 16 == 4 * entered, (placement, self.view.data_ptr() % 16)

  def check(self, what=''):
    s = SENTINEL[self.buf.dtype]
    before, after = self.buf[:self.lead].cpu(), self.buf[self.lead + self.n:].cpu()
    assert bool((before == s).all()), f'{what}: written before the view: {before.tolist()}'
    assert bool((after == s).all()), f'{what}: written past the view: {after.tolist()}'


def case_id(v):
  """Parametrize id of a (shape, shifted) case: '2x3x8x8' for the shape, 'aligned' / 'entered-one-in' for the flag."""
  return 'x'.join(map(str, v)) if isinstance(v, tuple) else ('entered-one-in' if v else 'aligned')


def stream():
  """The raw handle of torch's current stream, as the C entries take it."""
  return torch.cuda.current_stream().cuda_stream


def ptr(t):
  """The device pointer of an optional operand: None (null) where it is absent."""
  return None if t is None else t.data_ptr()


def nan(shape, dev, shifted=False):
  """An output buffer full of NaN, placed like an operand: whatever a launch leaves unwritten shows."""
  return place(torch.full(shape, float('nan')), dev, shifted)


# vector path; n = 315, scalar path; one element; a 16-byte-aligned buffer entered one element in (scalar path); 3072 blocks
# of vector items against stk_ew_grid's cap of 2048 (the grid strides); the same entered one element in (scalar grid strides)
SHAPES = [((2, 3, 8, 8), False), ((3, 3, 5, 7), False), ((1, 1, 1, 1), False), ((2, 3, 8, 8), True),
          ((16, 3, 256, 256), False), ((16, 3, 256, 256), True)]
# ... and for the per-sample kernels: 48 blocks share each row; 3000 rows of 4 stride the 2048 rows of the grid
ROW_SHAPES = SHAPES + [((4, 3, 256, 256), False), ((3000, 1, 2, 2), False)]


def drawn_operands(cases=ROW_SHAPES, scales=(1.5, 2.0, 1.0, 0.8)):
  """One fp32 tensor per scale and per shape of `cases` on the host (numpy), drawn from a seed the shape gives."""
  out = {}
  for shape in sorted({s for s, _ in cases}):
    rng = np.random.RandomState(sum(shape))
    out[shape] = [(rng.standard_normal(shape) * scale).astype(np.float32) for scale in scales]
  return out
