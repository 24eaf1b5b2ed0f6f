"""DPM-Solver++ (data prediction; order 1 = DDIM, order 2 = multistep 2M) restated in numpy from the published formulas
(Lu et al. 2022, Algorithm 2 and eq. 9): the reference of tests/test_dpm_solver_cpu.py and tests/test_gpu_dpm_solver.py.
It shares nothing with soft-truncation_amd/dpm_solver.py: the noise schedules are written out per family with closed-form
inverses of lambda, where the package inverts numerically through sde.marginal_prob.

  lambda_t = log(alpha_t / sigma_t),  h_i = lambda_{i+1} - lambda_i,  r_i = h_{i-1} / h_i
  d_i      = (x_i + sigma_i^2 score_i) / alpha_i
  D_i      = d_i                                      first order
  D_i      = d_i + (d_i - d_{i-1}) / (2 r_i)          second order
  x_{i+1}  = (sigma_{i+1} / sigma_i) x_i - alpha_{i+1} (exp(-h_i) - 1) D_i

`update` and `sample` take the working dtype: float64 is the reference, float32 (every operation rounded, no fused
multiply-add) measures what fp32 arithmetic alone does to the same recurrence.
"""
import numpy as np


class VP:
  """alpha = exp(-1/4 t^2 (b1 - b0) - 1/2 t b0), sigma = sqrt(1 - alpha^2)."""
  name = 'VPSDE'

  def __init__(self, beta_min=0.1, beta_max=20.):
    self.b0, self.b1 = float(beta_min), float(beta_max)

  def log_alpha(self, t):
    return -0.25 * t ** 2 * (self.b1 - self.b0) - 0.5 * t * self.b0

  def alpha_sigma(self, t):
    la = self.log_alpha(np.asarray(t, dtype=np.float64))
    return np.exp(la), np.sqrt(1. - np.exp(2. * la))

  def _time_of_log_alpha(self, la):
    b = 0.5 * self.b0
    return -2. * la / (b + np.sqrt(b * b - (self.b1 - self.b0) * la))

  def inverse_lambda(self, lam):
    return self._time_of_log_alpha(-0.5 * np.logaddexp(0., -2. * lam))        # alpha^2 = 1 / (1 + exp(-2 lambda))


class SubVP(VP):
  """alpha as VP, sigma = 1 - alpha^2."""
  name = 'subVPSDE'

  def alpha_sigma(self, t):
    la = self.log_alpha(np.asarray(t, dtype=np.float64))
    return np.exp(la), 1. - np.exp(2. * la)

  def inverse_lambda(self, lam):
    e = np.exp(lam)                                   # alpha / (1 - alpha^2) = e:  alpha = 2 e / (1 + sqrt(1 + 4 e^2))
    return self._time_of_log_alpha(np.log(2. * e / (1. + np.sqrt(1. + 4. * e * e))))


class VE:
  """alpha = 1, sigma = smin (smax / smin)^t."""
  name = 'VESDE'

  def __init__(self, sigma_min=0.01, sigma_max=50.):
    self.lo, self.hi = float(sigma_min), float(sigma_max)

  def alpha_sigma(self, t):
    t = np.asarray(t, dtype=np.float64)
    return np.ones_like(t), self.lo * (self.hi / self.lo) ** t

  def inverse_lambda(self, lam):
    return (-lam - np.log(self.lo)) / (np.log(self.hi) - np.log(self.lo))


def lam_of(fam, t):
  a, s = fam.alpha_sigma(t)
  return np.log(a) - np.log(s)


def fp32(v):
  return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def schedule(fam, steps, order=2, skip='logsnr', eps=1e-3, T=1., lower_order_final=True):
  """dict(times, alpha, sigma, lam, h, orders, coeffs [steps, 5] = (cx, cs, g, A, B), final).  The times are rounded to fp32
  before anything is computed from them."""
  t_hi, t_lo = float(fp32(T)), float(fp32(eps))
  if skip == 'logsnr':
    times = fam.inverse_lambda(np.linspace(lam_of(fam, t_hi), lam_of(fam, t_lo), steps + 1))
  elif skip == 'time':
    times = np.linspace(t_hi, t_lo, steps + 1)
  elif skip == 'time_quadratic':
    times = np.linspace(np.sqrt(t_hi), np.sqrt(t_lo), steps + 1) ** 2
  else:
    raise ValueError(skip)
  times = fp32(times)
  times[0], times[-1] = t_hi, t_lo
  alpha, sigma = fam.alpha_sigma(times)
  lam = np.log(alpha) - np.log(sigma)
  h = lam[1:] - lam[:-1]
  orders = [1] * steps
  if order == 2:
    for i in range(1, steps):
      orders[i] = 2
    if lower_order_final and steps < 15:
      orders[-1] = 1
  rows = []
  for i in range(steps):
    g = 0. if orders[i] == 1 else 1. / (2. * (h[i - 1] / h[i]))
    rows.append((1. / alpha[i], sigma[i] ** 2 / alpha[i], g, sigma[i + 1] / sigma[i], -alpha[i + 1] * np.expm1(-h[i])))
  final = np.array([1. / alpha[-1], sigma[-1] ** 2 / alpha[-1], 0., 0., 1.])
  return dict(times=times, alpha=alpha, sigma=sigma, lam=lam, h=h, orders=np.array(orders), coeffs=np.array(rows), final=final)


def update(x, score, d_prev, row, clip=None, dtype=np.float64):
  """One step on arrays of `dtype`, the coefficients rounded to it first -> (x_out, d)."""
  cx, cs, g, A, B = (dtype(v) for v in row)
  d = cx * x + cs * score
  if clip is not None:
    d = np.minimum(np.maximum(d, dtype(clip[0])), dtype(clip[1]))
  D = d if d_prev is None else d + g * (d - d_prev)
  out = A * x + B * D
  assert out.dtype == dtype and d.dtype == dtype
  return out, d


def sample(score, x, sched, clip=None, denoise=False, dtype=np.float64):
  """The loop: score(x, i) is the score at sched['times'][i] as an array of `dtype`.  -> x at eps (the data prediction there
  with denoise)."""
  x = x.astype(dtype)
  rows = list(sched['coeffs']) + ([sched['final']] if denoise else [])
  d_prev = None
  for i, row in enumerate(rows):
    x, d_prev = update(x, score(x, i).astype(dtype), d_prev if row[2] != 0. else None, row, clip, dtype)
  return x


class Gaussian:
  """Per-element data N(mu, c^2): the score of its diffused marginal and the exact probability flow, both closed-form."""

  def __init__(self, shape, seed=0):
    rng = np.random.RandomState(seed)
    self.mu = rng.uniform(-.5, .5, size=shape)
    self.c = rng.uniform(.1, .6, size=shape)

  def var(self, alpha, sigma):
    return alpha ** 2 * self.c ** 2 + sigma ** 2

  def score(self, x, alpha, sigma):
    return -(x - alpha * self.mu) / self.var(alpha, sigma)

  def flow(self, x_T, alpha_T, sigma_T, alpha, sigma):
    return alpha * self.mu + np.sqrt(self.var(alpha, sigma) / self.var(alpha_T, sigma_T)) * (x_T - alpha_T * self.mu)

  def prior(self, alpha_T, sigma_T, seed=1):
    """A draw of the exact marginal at T."""
    return alpha_T * self.mu + np.sqrt(self.var(alpha_T, sigma_T)) * np.random.RandomState(seed).standard_normal(self.mu.shape)


def gaussian_run(fam, gauss, steps, order, dtype=np.float64, eps=1e-3, T=1., lower_order_final=True, x_T=None):
  """(solver result, exact flow) at eps from x_T (default: one draw of the marginal at T), logsnr spacing."""
  s = schedule(fam, steps, order=order, skip='logsnr', eps=eps, T=T, lower_order_final=lower_order_final)
  a, sg = s['alpha'], s['sigma']
  x_T = gauss.prior(a[0], sg[0]) if x_T is None else np.asarray(x_T, dtype=np.float64)
  mu, c2 = gauss.mu.astype(dtype), (gauss.c ** 2).astype(dtype)

  def score(x, i):
    ai, var = dtype(a[i]), dtype(a[i] ** 2) * c2 + dtype(sg[i] ** 2)
    return -(x - ai * mu) / var

  return sample(score, x_T, s, dtype=dtype), gauss.flow(x_T, a[0], sg[0], a[-1], sg[-1])


def rel(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / np.abs(b).max())
