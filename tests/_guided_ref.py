"""Dynamic thresholding and guidance rescale (include/stk_guided.h) restated in numpy: the reference of
tests/test_guided_cpu.py, tests/test_gpu_guided.py and tests/test_gpu_guided_sampler.py.  It shares nothing with
soft-truncation_amd/dpm_solver.py or csrc/guided.hip: the order statistic is a full sort, the standard deviations are
numpy's two-pass float64 ones.

  q[b]  = sort(|v[b]|)[rank]                       rank = min(n - 1, ceil(p (n - 1)))
  s     = max(q, floor), NaN where q is NaN
  d     = clamp(cx x + cs score, -s, s) / s
  D     = d + g (d - d_prev),  x_out = A x + B D
  out   = (phi std(c) / std(g) + 1 - phi) g,       g = c + w (c - u), population std per row; factor 1 where std(g) = 0
"""
import math

import numpy as np

import _dpm_ref as R

U = 2.0 ** -24
K_D, K_X = 4, 9             # the plain update's 3 and 8 (tests/test_gpu_dpm_solver.py) and the division by s
K_RESCALE = 3               # f to fp32, the product, and one for the float64 variance
# (B, n) and whether the buffer is entered one element in: the smallest shapes at which each path can go wrong
SHAPES = [((1, 1), False),          # a single element
          ((2, 192), False),        # vector path
          ((3, 315), False),        # rows not a multiple of 4: scalar path
          ((2, 192), True),         # misaligned: scalar path
          ((2, 12288), False),      # several blocks share a row
          ((3000, 4), False)]       # more rows than the grid walks at once
CONTENTS = ('gaussian', 'equal', 'straddle', 'low-bits', 'exponents', 'specials', 'one-nan')


def rank_of(p, n):
  return min(n - 1, int(math.ceil(p * (n - 1))))


def ranks(n):
  """0, n - 1 and the ranks of p = 0.995 and p = 0.5, without repeats, ascending."""
  return sorted({0, n - 1, rank_of(0.995, n), rank_of(0.5, n)})


def select(v, rank):
  """sort(|v[b]|)[rank] per row of a float32 [B, n] array, as float32 (numpy sorts NaN last)."""
  assert v.dtype == np.float32 and v.ndim == 2
  return np.sort(np.abs(v), axis=1)[:, rank].copy()


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def content(kind, B, n, seed=0):
  """A float32 [B, n] array of one of CONTENTS."""
  rng = np.random.RandomState(seed + 17 * n + B)
  if kind == 'gaussian':
    return (rng.standard_normal((B, n)) * 1.7).astype(np.float32)
  if kind == 'equal':
    return np.full((B, n), -0.8125, dtype=np.float32)
  if kind == 'straddle':                         # one value repeated n // 2 times around the middle ranks, signs mixed
    v = (rng.standard_normal((B, n)) * 1.7).astype(np.float32)
    for b in range(B):
      order = np.argsort(np.abs(v[b]), kind='stable')
      lo = (n - n // 2) // 2
      mid = order[lo:lo + n // 2]
      if mid.size:
        v[b, mid] = np.abs(v[b, mid[0]]) * np.where(rng.rand(mid.size) < 0.5, -1, 1).astype(np.float32)
    return v
  if kind == 'low-bits':                         # one exponent, the upper 13 mantissa bits fixed: the last level decides
    low = rng.randint(0, 1024, size=(B, n)).astype(np.uint32)
    sign = (rng.randint(0, 2, size=(B, n)).astype(np.uint32)) << np.uint32(31)
    return (np.uint32(0x3fa5a400) | low | sign).view(np.float32)
  if kind == 'exponents':                        # one mantissa, exponents spread: the first level decides
    e = rng.randint(1, 255, size=(B, n)).astype(np.uint32)
    sign = (rng.randint(0, 2, size=(B, n)).astype(np.uint32)) << np.uint32(31)
    return ((e << np.uint32(23)) | np.uint32(0x2aaaab) | sign).view(np.float32)
  if kind == 'specials':
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, np.inf, -np.inf, 1.0, -2.5, 1.1754944e-38, 3.4028235e38],
                    dtype=np.float32)
    return pool[rng.randint(0, pool.size, size=(B, n))]
  if kind == 'one-nan':
    v = (rng.standard_normal((B, n)) * 1.7).astype(np.float32)
    v[0, (n - 1) // 2] = np.float32('nan')
    return v
  raise ValueError(kind)


# ---- the thresholded solver step -------------------------------------------------------------------------------------------
def predict32(x, score, cx, cs):
  """d_raw in fp32: each product rounded, then the sum (no fused multiply-add)."""
  f = np.float32
  out = (f(cx) * x).astype(f) + (f(cs) * score).astype(f)
  assert out.dtype == f
  return out


def scale_of(q, floor):
  """s = max(q, floor), NaN where q is NaN; dtype of q."""
  return np.where(np.isnan(q), q, np.maximum(q, q.dtype.type(floor)))


def threshold(d_raw, s):
  """clamp(d_raw, -s, s) / s with s [B] broadcast over the rows; a NaN s makes the row NaN."""
  s = s.reshape((-1,) + (1,) * (d_raw.ndim - 1))
  with np.errstate(invalid='ignore'):
    return np.minimum(np.maximum(d_raw, -s), s) / s


def step64(x, score, d_prev, row, s):
  """The thresholded step on float64 arrays [B, n], s [B] the scale in force -> (x_out, d, B_x, B_d): the results and the
  same expressions on absolute values (the magnitudes of the forward error bound)."""
  cx, cs, g, A, B = row
  d = threshold(cx * x + cs * score, s)
  D = d if d_prev is None else d + g * (d - d_prev)
  b_d = (abs(cx) * np.abs(x) + abs(cs) * np.abs(score)) / s.reshape(-1, 1)
  b_D = b_d if d_prev is None else b_d + abs(g) * (b_d + np.abs(d_prev))
  return A * x + B * D, d, abs(A) * np.abs(x) + abs(B) * b_D, b_d


def update(x, score, d_prev, row, p, floor, dtype=np.float64):
  """One thresholded step on arrays [B, ...] of `dtype`, coefficients rounded to it first -> (x_out, d, active) with
  active[b] = the quantile exceeded the floor."""
  cx, cs, g, A, B = (dtype(v) for v in row)
  d_raw = cx * x + cs * score
  flat = np.abs(d_raw.reshape(d_raw.shape[0], -1))
  q = np.sort(flat, axis=1)[:, rank_of(p, flat.shape[1])]
  d = threshold(d_raw, scale_of(q, floor))
  D = d if d_prev is None else d + g * (d - d_prev)
  out = A * x + B * D
  assert out.dtype == dtype and d.dtype == dtype
  return out, d, q > floor


def sample(score, x, sched, p, floor, denoise=False, dtype=np.float64):
  """The thresholded loop (tests/_dpm_ref.py sample with update above) -> (x, fraction of (step, sample) pairs on which
  the quantile exceeded the floor)."""
  x = x.astype(dtype)
  rows = list(sched['coeffs']) + ([sched['final']] if denoise else [])
  d_prev, active = None, []
  for i, row in enumerate(rows):
    x, d_prev, a = update(x, score(x, i).astype(dtype), d_prev if row[2] != 0. else None, row, p, floor, dtype)
    active.append(a)
  return x, float(np.mean(active))


# ---- guidance rescale ---------------------------------------------------------------------------------------------------------
def combine32(c, u, w):
  """g = c + w (c - u) in fp32, three roundings."""
  f = np.float32
  g = c + (f(w) * (c - u).astype(f)).astype(f)
  assert g.dtype == f
  return g


def rescale_factor(c, g, phi):
  """f[b] in float64 from float32 [B, n] rows: phi std(c) / std(g) + 1 - phi, 1 where std(g) is not finite and positive."""
  sd_c, sd_g = np.std(c.astype(np.float64), axis=1), np.std(g.astype(np.float64), axis=1)
  ok = np.isfinite(sd_g) & (sd_g > 0)
  return np.where(ok, phi * sd_c / np.where(ok, sd_g, 1.) + (1. - phi), 1.)


def rescale64(c, u, w, phi):
  """(out in float64, g in fp32, f in float64): the restatement computed from the fp32 g."""
  g = combine32(c, u, w)
  f = rescale_factor(c, g, float(np.float32(phi)))
  return f[:, None] * g.astype(np.float64), g, f


def rescale_operands(B, n, seed=0, constant_row=None):
  """(c, u) float32 [B, n] with |mean| <= 10 std per row (tests/test_guided_cpu.py checks it of c and of g)."""
  rng = np.random.RandomState(seed + 31 * n + B)

  def standard(z):                               # rows of mean 0 and std 1 (left alone where a row is constant: n = 1)
    z = z - z.mean(axis=1, keepdims=True)
    sd = z.std(axis=1, keepdims=True)
    return z / np.where(sd > 0, sd, 1.)

  c = standard(rng.standard_normal((B, n))) * 0.9 + rng.uniform(-2, 2, size=(B, 1))
  u = 0.7 * c + standard(rng.standard_normal((B, n))) * 0.5
  c, u = c.astype(np.float32), u.astype(np.float32)
  if constant_row is not None:
    c[constant_row], u[constant_row] = np.float32(0.375), np.float32(0.375)
  return c, u


# ---- a closed-form score whose data prediction leaves [-1, 1]: thresholding is active ---------------------------------------
class WideGaussian(R.Gaussian):
  """tests/_dpm_ref.py's Gaussian with means and widths scaled up, so |data prediction| passes 0.5 on most steps."""

  def __init__(self, shape, seed=0):
    super().__init__(shape, seed)
    self.mu = self.mu * 3.0
    self.c = self.c * 1.5
