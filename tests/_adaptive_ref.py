"""The adaptive-step SDE solver of Jolicoeur-Martineau et al. ("Gotta Go Fast When Generating Data with Score-Based Models",
2021, Algorithm 1) restated in numpy: the reference of tests/test_adaptive_sde_cpu.py and tests/test_gpu_adaptive_sde.py.
It shares nothing with soft-truncation_amd/adaptive_sde.py: drift and diffusion are written out per family in closed form,
where the package reads them from sde.sde.

With the forward SDE dx = c(t) x dt + g(t) dw, per sample b with its own t, h and t' = t - h:

  x1  = (1 - h c(t)) x + h g(t)^2 s1 + sqrt(h) g(t) z           s1 = score(x, t)
  xt  = x - h c(t') x1 + h g(t')^2 s2 + sqrt(h) g(t') z          s2 = score(x1, t')
  x2  = (x1 + xt) / 2
  d   = max(atol, rtol max(|x1|, |x1_prev|))
  E   = sqrt(mean((x1 - x2)^2 / d^2))                           over the sample's elements
  E <= 1: x <- x2, x1_prev <- x1, t <- t'                        otherwise nothing moves
  h   <- min(t - eps, safety h E^-exponent)                     with the new t

A step with h >= t - eps lands on eps itself; a sample at eps is finished: h = 0 and nothing of it changes any more.

Every function takes the working dtype: float64 is the reference, float32 (every operation rounded once, no fused
multiply-add, sums in numpy's pairwise order) measures what fp32 arithmetic alone does to the same expressions.
"""
import numpy as np


class VP:
  """beta(t) = b0 + t (b1 - b0): c = -beta / 2, g = sqrt(beta); alpha = exp(-1/4 t^2 (b1 - b0) - 1/2 t b0), sigma^2 = 1 - alpha^2."""
  name = 'VPSDE'

  def __init__(self, beta_min=0.1, beta_max=20.):
    self.b0, self.b1 = float(beta_min), float(beta_max)

  def beta(self, t):
    return self.b0 + t * (self.b1 - self.b0)

  def c(self, t):
    return -0.5 * self.beta(t)

  def g(self, t):
    return np.sqrt(self.beta(t))

  def alpha_sigma(self, t):
    la = -0.25 * t ** 2 * (self.b1 - self.b0) - 0.5 * t * self.b0
    return np.exp(la), np.sqrt(1. - np.exp(2. * la))


class SubVP(VP):
  """c as VP; g^2 = beta (1 - exp(-2 b0 t - (b1 - b0) t^2)); sigma = 1 - alpha^2."""
  name = 'subVPSDE'

  def g(self, t):
    return np.sqrt(self.beta(t) * (1. - np.exp(-2. * self.b0 * t - (self.b1 - self.b0) * t ** 2)))

  def alpha_sigma(self, t):
    a, s = VP.alpha_sigma(self, t)
    return a, s * s


class VE:
  """sigma(t) = lo (hi / lo)^t: c = 0, g = sigma(t) sqrt(2 log(hi / lo)); alpha = 1."""
  name = 'VESDE'

  def __init__(self, sigma_min=0.01, sigma_max=50.):
    self.lo, self.hi = float(sigma_min), float(sigma_max)

  def c(self, t):
    return np.zeros_like(t)

  def g(self, t):
    return self.lo * (self.hi / self.lo) ** t * np.sqrt(2. * (np.log(self.hi) - np.log(self.lo)))

  def alpha_sigma(self, t):
    return np.ones_like(t), self.lo * (self.hi / self.lo) ** t


class RVE:
  """sigma(t)^2 = k b^(2/t) + k2 b2^(2/t) on the horizon 1 / 1e-5: c = 0 and
  g^2 = (-2 k log(b) b^(2/t) + 2 k2 log(b2) b2^(2/t)) / t^2, the diffusion as the SDE defines it (its second component enters
  with the opposite sign of d sigma^2 / dt; it is 1e-11 of the first)."""
  name = 'reciprocal_VESDE'

  def __init__(self, eta=1e-5, sigma_min=0.01, sigma_max=50.):
    H = 1. / 1e-5
    self.b = (eta / sigma_max) ** (1. / (H - 1.))
    self.k = sigma_max ** 2 / self.b ** 2
    self.b2 = 1.01 ** (-1. / (2. * (H - 1.)))
    self.k2 = -(1.01 ** (H / (H - 1.))) * (eta ** 2 - sigma_min ** 2)

  def c(self, t):
    return np.zeros_like(t)

  def g(self, t):
    return np.sqrt((-2. * self.k * np.log(self.b) * self.b ** (2. / t) + 2. * self.k2 * np.log(self.b2) * self.b2 ** (2. / t)) / t ** 2)


def stage_row(fam, t, h, dtype=np.float64):
  """[B, 4]: (1 - h c(t), 0, h g(t)^2, sqrt(h) g(t)), from t and h of `dtype`."""
  t, h = t.astype(dtype), h.astype(dtype)
  c, g = fam.c(t).astype(dtype), fam.g(t).astype(dtype)
  return np.stack([1 - h * c, np.zeros_like(h), h * g * g, np.sqrt(h) * g], axis=1).astype(dtype)


def heun_row(fam, t_next, h, dtype=np.float64):
  """[B, 4]: (1, -h c(t'), h g(t')^2, sqrt(h) g(t'))."""
  t, h = t_next.astype(dtype), h.astype(dtype)
  c, g = fam.c(t).astype(dtype), fam.g(t).astype(dtype)
  return np.stack([np.ones_like(h), -(h * c), h * g * g, np.sqrt(h) * g], axis=1).astype(dtype)


def _col(row, k, x):
  return row[:, k].reshape((-1,) + (1,) * (x.ndim - 1))


def stage(x, xp, score, z, row):
  """(a x + p xp) + s score + n z per sample, in the dtype of the operands; xp None leaves its term out."""
  r = _col(row, 0, x) * x
  if xp is not None:
    r = r + _col(row, 1, x) * xp
  r = r + _col(row, 2, x) * score
  return r + _col(row, 3, x) * z


def heun_error(x, x1, x1_prev, score2, z, row, atol, rtol):
  """-> (x2, E [B]) in the dtype of the operands."""
  dtype = x.dtype.type
  xt = stage(x, x1, score2, z, row)
  x2 = dtype(0.5) * (x1 + xt)
  d = np.maximum(dtype(atol), dtype(rtol) * np.maximum(np.abs(x1), np.abs(x1_prev)))
  q = (x1 - x2) / d
  E = np.sqrt(np.mean((q * q).reshape(x.shape[0], -1), axis=1, dtype=dtype))
  assert x2.dtype == x.dtype and E.dtype == x.dtype
  return x2, E


def next_time(t, h, eps):
  return np.where(h >= t - eps, eps, t - h).astype(t.dtype)


def controller(t, h, E, eps, safety, exponent):
  """-> (accept [B] bool, t_new, h_new) by the rules of the module docstring; a non-finite E rejects and halves the step."""
  dtype = t.dtype.type
  eps = dtype(eps)
  active = t > eps
  finite = np.isfinite(E)
  with np.errstate(all='ignore'):
    accept = active & (E <= 1)
    t_new = np.where(accept, next_time(t, h, eps), t).astype(dtype)
    factor = np.where(finite, np.power(E.astype(np.float64), -float(exponent)), 0.5)
    grown = (float(safety) * h.astype(np.float64) * factor).astype(dtype)
    h_new = np.where(active, np.fmin(t_new - eps, grown), 0).astype(dtype)
  return accept, t_new, h_new


def sample(score, x, fam, noise, rtol, atol, h_init=0.01, safety=0.9, exponent=0.9, eps=1e-3, T=1., max_iters=10000,
           dtype=np.float64, watch=None):
  """The loop.  score(x, t [B]) -> array; noise(shape) -> one standard normal draw per iteration.  -> (x, iterations, info)
  with info = dict(accepted, rejected [B] counts, E, accept: per-iteration lists, t).  watch(iteration, x, t, h) is called
  at the top of every iteration.  RuntimeError when max_iters iterations leave a sample above eps."""
  x = x.astype(dtype)
  B = x.shape[0]
  eps, T = dtype(np.float32(eps)), dtype(np.float32(T))
  t = np.full(B, T, dtype=dtype)
  h = np.minimum(np.full(B, h_init, dtype=dtype), t - eps)
  x1_prev = x.copy()
  accepted, rejected = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
  Es, accepts = [], []
  iterations = 0
  while not (t <= eps).all():
    if iterations >= max_iters:
      raise RuntimeError(f'not at eps after {max_iters} iterations')
    if watch is not None:
      watch(iterations, x, t, h)
    z = noise(x.shape).astype(dtype)
    x1 = stage(x, None, score(x, t).astype(dtype), z, stage_row(fam, t, h, dtype))
    t_next = next_time(t, h, eps)
    x2, E = heun_error(x, x1, x1_prev, score(x1, t_next).astype(dtype), z, heun_row(fam, t_next, h, dtype), atol, rtol)
    accept, t_new, h_new = controller(t, h, E, eps, safety, exponent)
    sel = accept.reshape((-1,) + (1,) * (x.ndim - 1))
    x, x1_prev = np.where(sel, x2, x), np.where(sel, x1, x1_prev)
    accepted += accept
    rejected += (t > eps) & ~accept
    Es.append(E)
    accepts.append(accept)
    t, h = t_new, h_new
    iterations += 1
  return x, iterations, dict(accepted=accepted, rejected=rejected, E=Es, accept=accepts, t=t, h=h)


class Gaussian:
  """Per-element data N(mu, s0^2): its diffused marginal at t is N(alpha mu, alpha^2 s0^2 + sigma^2), and the score of that
  is closed-form."""

  def __init__(self, mu, s0):
    self.mu, self.s0 = mu, s0

  def var(self, alpha, sigma):
    return alpha ** 2 * self.s0 ** 2 + sigma ** 2

  def score_fn(self, fam, dtype=np.float64):
    def score(x, t):
      a, s = fam.alpha_sigma(t.astype(np.float64))
      shape = (-1,) + (1,) * (x.ndim - 1)
      a, s = a.reshape(shape), s.reshape(shape)
      return (-(x - a.astype(dtype) * dtype(self.mu)) / self.var(a, s).astype(dtype)).astype(dtype)
    return score


def rel(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / np.abs(b).max())
