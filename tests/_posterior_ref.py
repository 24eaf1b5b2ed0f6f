"""The restatement of include/stk_posterior.h that the posterior-sampling tests compare with: the four entries, the magnitudes B
of their rounding bounds k 2^-24 B, the measurement operators in plain torch, a closed-form score, and a guided step.

Everything is torch on the host and takes its precision from its operands: float64 operands give the reference, float32
operands the plain fp32 restatement the entries reproduce bit for bit (torch rounds every product, quotient and sum once).
State tensors are [N, ...]; a, s, rnorm are [N].

Roundings on the longest path to each result (u = 2^-24; the tests hold K = k + 1, since gamma_k = k u / (1 - k u) < (k + 1) u):
  x0    = (x + (s s) score) / a     s s, the product, the sum, the quotient (correctly rounded in this build): k = 4; the
                                    clamp moves no value further from the exact clamped one
  r     = y - m                     k = 1
  seed  = ((s s) / a) v             k = 3
  x_out = xp + (zeta / rnorm) g,  g = v / a + gnet      the quotient and the sum of g (2), the quotient of c (1), their product
                                    (1), the last sum (1): k = 5
"""
import math

import torch
import torch.nn.functional as F

K_X0, K_R, K_SEED, K_OUT = 5, 2, 4, 6
INF = math.inf


def wide(v, like):
  return v.reshape((-1,) + (1,) * (like.dim() - 1))


def inside(x0, lo, hi):
  return (x0 > lo) & (x0 < hi)


# ---- the four entries ---------------------------------------------------------------------------------------------------
def tweedie(x, score, a, s, lo=-INF, hi=INF):
  s2 = wide(s * s, x)
  return ((x + s2 * score) / wide(a, x)).clamp(lo, hi)


def tweedie_mag(x, score, a, s):
  return (x.abs() + wide(s * s, x) * score.abs()) / wide(a.abs(), x)


def residual(y, m):
  """(r, rnorm): rnorm is the root of the float64 sum of r r, each square rounded in r's precision."""
  r = y - m
  rr = (r * r).double().reshape(r.shape[0], -1).sum(dim=1)
  return r, rr.sqrt()


def seed(v, x0, a, s, lo=-INF, hi=INF):
  c = wide((s * s) / a, v)
  return torch.where(inside(x0, lo, hi), c * v, torch.zeros_like(v))


def seed_mag(v, a, s):
  return wide((s * s) / a.abs(), v) * v.abs()


def guide(v, gnet, x0, a, lo=-INF, hi=INF):
  return torch.where(inside(x0, lo, hi), v / wide(a, v) + gnet, gnet)


def step_size(rnorm, zeta):
  ok = (rnorm > 0) & torch.isfinite(rnorm)
  return torch.where(ok, zeta / torch.where(ok, rnorm, torch.ones_like(rnorm)), torch.zeros_like(rnorm))


def update(xp, v, gnet, x0, a, rnorm, zeta, lo=-INF, hi=INF):
  """xp + c g; the same expression serves x_mean with xpm in place of xp."""
  zeta = torch.tensor(zeta, dtype=xp.dtype)
  return xp + wide(step_size(rnorm, zeta), xp) * guide(v, gnet, x0, a, lo, hi)


def update_mag(xp, v, gnet, a, rnorm, zeta):
  c = step_size(rnorm.double(), torch.tensor(zeta, dtype=torch.float64))
  return xp.abs() + wide(c, xp) * (v.abs() / wide(a.abs(), v) + gnet.abs())


# ---- operators, restated in plain torch ------------------------------------------------------------------------------------
def gaussian_taps(size, std, rounded=False):
  """float64 [size, size] taps of a sampled Gaussian, sum 1; rounded: the values after one rounding to fp32."""
  i = torch.arange(size, dtype=torch.float64) - (size - 1) / 2
  g = torch.exp(-(i * i) / (2 * std * std))
  k = g[:, None] * g[None, :]
  k = k / k.sum()
  return k.float().double() if rounded else k


def blur(size, std, rounded=False):
  taps = gaussian_taps(size, std, rounded)
  before, after = size // 2, (size - 1) // 2

  def A(x0):
    C = x0.shape[1]
    w = taps.to(x0.dtype)[None, None].expand(C, 1, size, size)
    return F.conv2d(F.pad(x0, (before, after, before, after)), w, groups=C)
  return A


def masking(mask):
  return lambda x0: x0 * mask.to(x0.dtype)


def block_average(r):
  return lambda x0: F.avg_pool2d(x0, r)


# ---- a closed-form score ---------------------------------------------------------------------------------------------------
def gaussian_score(mu, tau, a, s):
  """The score of x_t = a x_0 + s z for data x_0 ~ N(mu, tau^2): -(x - a mu) / (a^2 tau^2 + s^2); a, s [N]."""
  def score(x, t=None):
    aw, sw = wide(a.to(x.dtype), x), wide(s.to(x.dtype), x)
    return -(x - aw * mu.to(x.dtype)) / (aw * aw * tau * tau + sw * sw)
  return score


# ---- a guided step ---------------------------------------------------------------------------------------------------------
def gradient_parts(score_of, A, y, x, a, s, lo=-INF, hi=INF):
  """(score, x0, r, rnorm, v, gnet) of one guided step in x's precision, by torch.autograd: score_of(x) -> the score."""
  with torch.enable_grad():
    xg = x.detach().clone().requires_grad_(True)
    score = score_of(xg)
    x0g = tweedie(x, score.detach(), a, s, lo, hi).requires_grad_(True)
    m = A(x0g)
    r, rnorm = residual(y, m.detach())
    v = torch.autograd.grad(m, x0g, r)[0]
    gnet = torch.autograd.grad(score, xg, seed(v, x0g.detach(), a, s, lo, hi))[0]
  return score.detach(), x0g.detach(), r, rnorm.to(x.dtype), v, gnet


def measurement_gradient(score_of, A, y, x, a, s, lo=-INF, hi=INF):
  """(g, rnorm, x0) as posterior_sampling.measurement_gradient states them."""
  _, x0, _, rnorm, v, gnet = gradient_parts(score_of, A, y, x, a, s, lo, hi)
  return guide(v, gnet, x0, a, lo, hi), rnorm, x0


def guided_step(score_of, A, y, x, a, s, zeta, xp, xpm, lo=-INF, hi=INF):
  """(x_out, x_mean, rnorm) of dps_update given the unconditional update's outputs (xp, xpm)."""
  _, x0, _, rnorm, v, gnet = gradient_parts(score_of, A, y, x, a, s, lo, hi)
  return update(xp, v, gnet, x0, a, rnorm, zeta, lo, hi), update(xpm, v, gnet, x0, a, rnorm, zeta, lo, hi), rnorm


def norm_gradient(score_of, A, y, x, a, s, lo=-INF, hi=INF):
  """d/dx of sum over samples of |y - A(clamp((x + s^2 score(x)) / a))|, differentiated as ONE expression: what g / rnorm must be
  the negative of."""
  with torch.enable_grad():
    xg = x.detach().clone().requires_grad_(True)
    x0 = ((xg + wide(s * s, xg) * score_of(xg)) / wide(a, xg)).clamp(lo, hi)
    res = y - A(x0)
    total = res.reshape(res.shape[0], -1).norm(dim=1).sum()
    return torch.autograd.grad(total, xg)[0]


def adjoint(A, like):
  """z -> A^T z for a linear A acting on tensors shaped like `like`, by autograd in z's precision."""
  def At(z):
    with torch.enable_grad():
      w = torch.zeros(like.shape, dtype=z.dtype, requires_grad=True)
      return torch.autograd.grad(A(w), w, z)[0]
  return At
