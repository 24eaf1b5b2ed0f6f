"""An independent numpy restatement of the EDM formulation (Karras et al. 2022, Table 1 column "Ours", Algorithm 2), which the
tests of soft-truncation_amd/edm.py, the EDM loss and csrc/edm.hip compare against.  Nothing here imports the package."""
import numpy as np

SQRT2M1 = np.sqrt(2.) - 1.


def fp32(v):
  return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def table1(sigma, s):
  """(c_in, c_skip, c_out, c_noise, lambda) of Table 1 at the float64 levels sigma, as the paper writes them."""
  sigma = np.asarray(sigma, dtype=np.float64)
  tot = sigma ** 2 + s ** 2
  c_out = sigma * s / np.sqrt(tot)
  return 1. / np.sqrt(tot), s ** 2 / tot, c_out, np.log(sigma) / 4., 1. / c_out ** 2


def coeff_rows(sigma32, s, dtype=np.float64):
  """The six rows of stk_edm_coeffs_f32 for fp32 levels, float64 in the header's operation order, rounded to `dtype` once."""
  S, d = np.asarray(sigma32, dtype=np.float32).astype(np.float64), float(np.float32(s))
  v = S * S + d * d
  q = np.sqrt(v)
  p = S * d
  with np.errstate(divide='ignore', invalid='ignore'):
    rows = [1. / q, S / q, (d * d) / v, p / q, v / (p * p), np.log(S) / 4.]
  return np.stack(rows).astype(dtype)


def sigmas(sigma_min, sigma_max, steps, rho=7.):
  """sigma_0 ... sigma_{steps-1} of the rho-schedule, then 0: each rounded to fp32."""
  lo, hi = float(np.float32(sigma_min)), float(np.float32(sigma_max))
  i = np.arange(steps, dtype=np.float64)
  sig = fp32((hi ** (1. / rho) + i / (steps - 1) * (lo ** (1. / rho) - hi ** (1. / rho))) ** rho)
  sig[0], sig[-1] = hi, lo
  return np.concatenate([sig, [0.]])


def churn(sig, steps, s_churn=0., s_tmin=0., s_tmax=np.inf, s_noise=1.):
  """(gamma, t_hat, c_eps) of the levels sig[:steps]."""
  sig = sig[:steps]
  gamma = np.where((sig >= s_tmin) & (sig <= s_tmax), min(s_churn / steps, SQRT2M1), 0.)
  t_hat = fp32(sig + gamma * sig)
  return gamma, t_hat, s_noise * np.sqrt(t_hat ** 2 - sig ** 2)


def heun(denoise, x, sig, s_churn=0., s_tmin=0., s_tmax=np.inf, s_noise=1., noise=None, dtype=np.float64):
  """Algorithm 2 on the levels `sig` (ending in 0) with denoise(x, sigma) -> D, every operation in `dtype`.  noise: the
  recorded eps of the churned steps, in step order."""
  steps = len(sig) - 1
  gamma, t_hat, c_eps = churn(sig, steps, s_churn, s_tmin, s_tmax, s_noise)
  x = np.asarray(x, dtype=dtype)
  noise = iter(noise or ())
  half = dtype(0.5)
  for i in range(steps):
    t, t_next = dtype(t_hat[i]), dtype(sig[i + 1])
    if t_hat[i] > sig[i]:
      x = x + dtype(c_eps[i]) * np.asarray(next(noise), dtype=dtype)
    h = dtype(sig[i + 1] - t_hat[i])
    d = (x - denoise(x, t)) / t
    x1 = x + h * d
    if sig[i + 1] > 0.:
      d1 = (x1 - denoise(x1, t_next)) / t_next
      x1 = x + h * (half * d + half * d1)
    x = x1
  return x


class GaussianData:
  """Per-element data N(mu, c^2): its exact denoiser, the raw network output F that yields it under the preconditioning with
  sigma_data = s, and the exact probability flow."""

  def __init__(self, shape, s=0.5, seed=0):
    rng = np.random.RandomState(seed)
    self.mu = rng.uniform(-.5, .5, size=shape)
    self.c = rng.uniform(.1, .6, size=shape)
    self.s = s

  def denoise(self, x, sigma):
    dt = x.dtype.type
    c2 = (self.c ** 2).astype(x.dtype)
    mu = self.mu.astype(x.dtype)
    return mu + c2 / (c2 + dt(sigma) * dt(sigma)) * (x - mu)

  def flow(self, x_T, sigma_T, sigma):
    return self.mu + np.sqrt((self.c ** 2 + sigma ** 2) / (self.c ** 2 + sigma_T ** 2)) * (x_T - self.mu)

  def prior(self, sigma_T, seed=1):
    return self.mu + np.sqrt(self.c ** 2 + sigma_T ** 2) * np.random.RandomState(seed).standard_normal(self.mu.shape)


def rel(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / np.abs(b).max())


def loss(F, y, n, sigma, s, reduce_mean):
  """The Table 1 training loss per sample, float64: lambda(sigma) |D(y + sigma n; sigma) - y|^2 with
  D = c_skip x + c_out F, summed (or averaged) over C H W.  F is the network output at (c_in x, c_noise)."""
  c_in, c_skip, c_out, c_noise, lam = table1(sigma, s)
  w = lambda v: v[:, None, None, None]
  x = y + w(sigma) * n
  r = w(c_skip) * x + w(c_out) * F - y
  total = (r * r).reshape(r.shape[0], -1)
  return lam * (total.mean(axis=1) if reduce_mean else total.sum(axis=1))


def gaussian_F(gauss, xin, sigma):
  """The raw network output that makes D the exact denoiser of `gauss`: F = (D(x) - c_skip x) / c_out at x = xin / c_in."""
  c_in, c_skip, c_out, _, _ = (xin.dtype.type(v) for v in table1(sigma, gauss.s))
  x = xin / c_in
  return (gauss.denoise(x, sigma) - c_skip * x) / c_out


def launch_loop(sch, F_of, x, noise=None, dtype=np.float64):
  """The loop of edm.edm_sample restated on the rows of an edm.EdmSchedule: the lines of include/stk_edm.h, every operation
  in `dtype`, F_of(xin, sigma) the network.  noise: the recorded eps of the churned steps, in step order."""
  c = dtype
  x = np.asarray(x, dtype=dtype)
  noise = iter(noise or ())
  half = c(0.5)
  xin = None
  for i in range(sch.steps):
    if sch.gamma[i] > 0.:
      x = x + c(sch.c_eps[i]) * np.asarray(next(noise), dtype=dtype)
      xin = c(sch.c_in_hat[i]) * x
    elif i == 0:
      xin = c(sch.c_in_hat[0]) * x
    cs, co, t, h, cn = (c(v) for v in sch.euler[i][:5])
    F = F_of(xin, float(sch.euler[i][2]))
    D = cs * x + co * F
    d = (x - D) / t
    x1 = x + h * d
    xin = cn * x1
    if i == sch.steps - 1:
      return x1
    cs, co, t, h, cn = (c(v) for v in sch.correct[i][:5])
    F = F_of(xin, float(sch.correct[i][2]))
    D = cs * x1 + co * F
    dn = (x1 - D) / t
    x = x + h * (half * d + half * dn)
    xin = cn * x
  return x
