"""An independent numpy restatement of consistency training and sampling (Song et al. 2023, "Consistency Models"; Song &
Dhariwal 2023, "Improved Techniques for Training Consistency Models"), which the tests of soft-truncation_amd/consistency.py,
the consistency loss and csrc/consistency.hip compare against.  Nothing here imports the package."""
import math

import numpy as np

RHO = 7.


def fp32(v):
  return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def rel(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / np.abs(b).max())


def boundary(sigma, s, e):
  """(c_in, c_skip, c_out, c_noise) of the consistency function at the float64 levels sigma, as the papers write them."""
  sigma = np.asarray(sigma, dtype=np.float64)
  tot = sigma ** 2 + s ** 2
  return 1. / np.sqrt(tot), s ** 2 / ((sigma - e) ** 2 + s ** 2), s * (sigma - e) / np.sqrt(tot), np.log(sigma) / 4.


def level_rows(sigma32, s, e, dtype=np.float64):
  """The five rows of one level of stk_ct_coeffs_f32 for fp32 levels, float64 in the header's operation order, rounded to
  `dtype` once: c_in, c_in sigma, c_skip, c_out, c_noise."""
  S, d, m = np.asarray(sigma32, dtype=np.float32).astype(np.float64), float(np.float32(s)), float(np.float32(e))
  v = S * S + d * d
  q = np.sqrt(v)
  g = S - m
  w = g * g + d * d
  with np.errstate(divide='ignore', invalid='ignore'):
    rows = [1. / q, S / q, (d * d) / w, (d * g) / q, np.log(S) / 4.]
  return np.stack(rows).astype(dtype)


def coeff_rows(hi32, lo32, s, e, dtype=np.float64):
  """The eleven rows of stk_ct_coeffs_f32: the five of sigma_hi, the five of sigma_lo, lambda = 1 / (sigma_hi - sigma_lo)."""
  hi, lo = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (hi32, lo32))
  with np.errstate(divide='ignore', invalid='ignore'):
    lam = (1. / (hi - lo))[None]
  return np.concatenate([level_rows(hi32, s, e), level_rows(lo32, s, e), lam]).astype(dtype)


def levels(sigma_min, sigma_max, N, rho=RHO):
  """sigma_1 < ... < sigma_N of the rho-grid, each rounded to fp32, the ends exact."""
  lo, hi = float(np.float32(sigma_min)), float(np.float32(sigma_max))
  out = []
  for i in range(1, N + 1):
    out.append((lo ** (1. / rho) + (i - 1) / (N - 1) * (hi ** (1. / rho) - lo ** (1. / rho))) ** rho)
  out = fp32(out)
  out[0], out[-1] = lo, hi
  return out


def num_levels(k, K, s0=10, s1=1280):
  per = int(math.floor(K / (math.log2(s1 / s0) + 1)))
  return min(s0 * 2 ** (k // per), s1) + 1


def index_pmf(lv, p_mean=-1.1, p_std=2.0):
  edge = [math.erf((math.log(v) - p_mean) / (math.sqrt(2.) * p_std)) for v in lv]
  raw = np.array([b - a for a, b in zip(edge[:-1], edge[1:])])
  return raw / raw.sum(), float(raw.sum())


def _w(v):
  return np.asarray(v).reshape(-1, 1, 1, 1)


def residual(F_hi, F_lo, y, n, hi, lo, s, e):
  """r = f(y + sigma_hi n; sigma_hi) - f(y + sigma_lo n; sigma_lo), float64, from the papers' coefficients."""
  _, ck_h, co_h, _ = boundary(hi, s, e)
  _, ck_l, co_l, _ = boundary(lo, s, e)
  f_hi = _w(ck_h) * (y + _w(hi) * n) + _w(co_h) * F_hi
  f_lo = _w(ck_l) * (y + _w(lo) * n) + _w(co_l) * F_lo
  return f_hi - f_lo


def loss(F_hi, F_lo, y, n, hi, lo, s, e, c, reduce_mean):
  """The pseudo-Huber consistency loss per sample, float64, in the form the papers write: lambda (sqrt(S + c^2) - c)."""
  r = residual(F_hi, F_lo, y, n, hi, lo, s, e)
  S = (r * r).reshape(r.shape[0], -1).sum(axis=1)
  out = (np.sqrt(S + c * c) - c) / (hi - lo)
  return out / r[0].size if reduce_mean else out


def loss_stable(F_hi, F_lo, y, n, hi, lo, s, e, c, reduce_mean):
  """... and in the cancellation-free form lambda S / (sqrt(S + c^2) + c)."""
  r = residual(F_hi, F_lo, y, n, hi, lo, s, e)
  S = (r * r).reshape(r.shape[0], -1).sum(axis=1)
  out = S / (np.sqrt(S + c * c) + c) / (hi - lo)
  return out / r[0].size if reduce_mean else out


def loss_grad(F_hi, F_lo, y, n, hi, lo, s, e, c, reduce_mean, dloss):
  """d (sum_b dloss_b loss_b) / d F_hi = (dloss lambda c_out_hi / sqrt(S + c^2)) r, float64."""
  r = residual(F_hi, F_lo, y, n, hi, lo, s, e)
  S = (r * r).reshape(r.shape[0], -1).sum(axis=1)
  co_h = boundary(hi, s, e)[2]
  k = dloss * co_h / ((hi - lo) * np.sqrt(S + c * c))
  if reduce_mean:
    k = k / r[0].size
  return _w(k) * r


class GaussianData:
  """Per-element data N(mu, c^2): the exact probability flow of the family x_t = x_0 + t z, which IS the consistency function
  f(x, sigma) = flow(x, sigma, sigma_min), and the raw network output F that yields it under the boundary-condition
  coefficients with sigma_data = s."""

  def __init__(self, shape, s=0.5, seed=0):
    rng = np.random.RandomState(seed)
    self.mu = rng.uniform(-.5, .5, size=shape)
    self.c = rng.uniform(.1, .6, size=shape)
    self.s = s

  def flow(self, x_T, sigma_T, sigma):
    dt = np.asarray(x_T).dtype.type
    c2, mu = (self.c ** 2).astype(dt), self.mu.astype(dt)
    return mu + np.sqrt((c2 + dt(sigma) * dt(sigma)) / (c2 + dt(sigma_T) * dt(sigma_T))) * (x_T - mu)

  def F(self, xin, sigma, e):
    """F = (f(x, sigma) - c_skip x) / c_out at x = xin / c_in, in xin's dtype.  sigma > e."""
    dt = xin.dtype.type
    c_in, c_skip, c_out, _ = (dt(v) for v in boundary(sigma, self.s, e))
    x = xin / c_in
    return (self.flow(x, sigma, e) - c_skip * x) / c_out


def sample_loop(F_of, lv, z, s, e, lo=-1., hi=1., dtype=np.float64):
  """The sampler on the strictly decreasing fp32 levels lv with the recorded standard normal draws z (len(lv) of them): the
  lines of include/stk_consistency.h, every operation in `dtype`; the per-launch scalars are float64 expressions of the fp32
  levels rounded to fp32 once, as the product hands them to the kernel.  F_of(xin, sigma) is the network."""
  c = dtype
  lv = [float(np.float32(v)) for v in lv]
  e = float(np.float32(e))
  rows = level_rows(lv, s, e, np.float32).astype(np.float64)
  x = c(np.float32(lv[0])) * np.asarray(z[0], dtype=dtype)
  xin = c(rows[0][0]) * x
  for j, sigma in enumerate(lv):
    F = F_of(xin, sigma)
    x0 = c(rows[2][j]) * x + c(rows[3][j]) * F
    x0 = np.where(x0 < c(lo), c(lo), x0)
    x0 = np.where(x0 > c(hi), c(hi), x0)
    if j == len(lv) - 1:
      return x0
    c_z = c(np.float32(math.sqrt(lv[j + 1] * lv[j + 1] - e * e)))
    x = x0 + c_z * np.asarray(z[j + 1], dtype=dtype)
    xin = c(rows[0][j + 1]) * x
