"""An independent numpy restatement of rectified flow -- the shifted time grid, the rows of the step launch, the lines of
include/stk_flow.h, the loops of soft-truncation_amd/flow.py, the loss, and the closed-form velocity of Gaussian data with the
variance recursion of the discrete sampler on it -- which the tests of flow.py, the flow loss and csrc/flow.hip compare
against.  Nothing here imports the package."""
import numpy as np


def fp32(v):
  return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def rel(a, b):
  a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
  return float(np.abs(a - b).max() / np.abs(b).max())


# ---- the schedule -----------------------------------------------------------------------------------------------------
def times(steps, shift=1.):
  """t_0 = 1 > ... > t_steps = 0: u_i = 1 - i / steps, t_i = shift u_i / (1 + (shift - 1) u_i), each rounded to fp32."""
  u = 1. - np.arange(steps + 1, dtype=np.float64) / steps
  t = fp32(shift * u / (1. + (shift - 1.) * u))
  t[0], t[-1] = 1., 0.
  return t


def rows(t, eta=0.):
  """(cx, cv, cn) per step of the times t: cx = 1 - e D, cv = -D (1 + e (1 - t_i)), cn = sqrt(2 e t_i D), with e = eta but 0
  on the last step."""
  steps = len(t) - 1
  out = np.empty((steps, 3))
  for i in range(steps):
    D = t[i] - t[i + 1]
    e = eta if i < steps - 1 else 0.
    out[i] = (1. - e * D, -D * (1. + e * (1. - t[i])), np.sqrt(2. * e * t[i] * D))
  return out


class Schedule:
  """What the loops below need of a schedule: built from this file's formulas, never from the package."""

  def __init__(self, steps, order=1, shift=1., eta=0.):
    self.steps, self.order = steps, order
    self.times = times(steps, shift)
    self.rows = rows(self.times, eta)
    self.nfe = steps if order == 1 else 2 * steps - 1


# ---- the lines of the header ------------------------------------------------------------------------------------------
def step(xb, v, v_prev, eps, row, dtype):
  """stk_flow_step_f32 in `dtype`, every operation rounded once -> (x_out, B): B is the same expression on absolute values."""
  cx, cv, cn = (dtype(c) for c in row)
  xb, v = xb.astype(dtype), v.astype(dtype)
  half = dtype(0.5)
  if v_prev is None:
    slope, b_s = v, np.abs(v)
  else:
    p = v_prev.astype(dtype)
    slope, b_s = half * p + half * v, half * np.abs(p) + half * np.abs(v)
  m = cx * xb
  p = cv * slope
  x = m + p
  mag = abs(cx) * np.abs(xb) + abs(cv) * b_s
  if eps is not None:
    e = eps.astype(dtype)
    x = x + cn * e
    mag = mag + abs(cn) * np.abs(e)
  return x, mag


def residual(F, y, n, dtype):
  """u = n - y;  r = F - u  in `dtype` -> (r, B)."""
  F, y, n = F.astype(dtype), y.astype(dtype), n.astype(dtype)
  u = n - y
  return F - u, np.abs(F) + np.abs(n) + np.abs(y)


def loss(F, y, n, reduce_mean):
  """The per-sample loss in float64: |F - (n - y)|^2 summed (or averaged) over C H W."""
  r = residual(F, y, n, np.float64)[0]
  total = (r * r).reshape(r.shape[0], -1)
  return total.mean(axis=1) if reduce_mean else total.sum(axis=1)


# ---- the loops ------------------------------------------------------------------------------------------------------------
def loop(sch, v_of, x, noise=None, dtype=np.float64):
  """flow.flow_sample restated on a Schedule: the header's lines, every operation in `dtype`; v_of(x, t) is the velocity at
  the float time t.  noise: the recorded eps of the stochastic steps, in step order."""
  x = np.asarray(x, dtype=dtype)
  noise = iter(noise or ())
  for i in range(sch.steps):
    row, t, t_next = sch.rows[i], float(sch.times[i]), float(sch.times[i + 1])
    v = v_of(x, t)
    if sch.order == 1 or i == sch.steps - 1:
      eps = np.asarray(next(noise), dtype=dtype) if row[2] > 0. else None
      x = step(x, v, None, eps, row, dtype)[0]
      continue
    x1 = step(x, v, None, None, row, dtype)[0]
    x = step(x, v_of(x1, t_next), v, None, row, dtype)[0]
  return x


# ---- Gaussian data ----------------------------------------------------------------------------------------------------
def gaussian_k(t, c):
  """For x_0 ~ N(0, c^2) the exact velocity is E[z - x_0 | x_t = x] = k(t) x:  k = (t - (1 - t) c^2) / ((1 - t)^2 c^2 + t^2)."""
  return (t - (1. - t) * c * c) / ((1. - t) ** 2 * c * c + t * t)


def gaussian_velocity(c):
  """v_of(x, t) of per-element data N(0, c^2), c an array of x's shape (or a scalar), in x's dtype."""
  def v_of(x, t):
    dt = x.dtype.type
    one, tt = dt(1.), dt(t)
    c2 = np.asarray(c * c, dtype=x.dtype)
    a = one - tt
    return (tt - a * c2) / (a * a * c2 + tt * tt) * x
  return v_of


def variance_recursion(sch, c):
  """The variance of the discrete sampler on x_0 ~ N(0, c^2) from Var = 1 at t = 1, float64: Var <- (cx + cv k)^2 Var + cn^2
  per Euler or stochastic step, and for a Heun step the composed multiplier 1 + cv (k_i / 2 + k_{i+1} (1 + cv k_i) / 2)."""
  var = 1.
  for i in range(sch.steps):
    cx, cv, cn = sch.rows[i]
    k = gaussian_k(sch.times[i], c)
    if sch.order == 1 or i == sch.steps - 1:
      var = (cx + cv * k) ** 2 * var + cn * cn
    else:
      m1 = 1. + cv * k
      m = 1. + cv * (0.5 * k + 0.5 * gaussian_k(sch.times[i + 1], c) * m1)
      var = m * m * var
  return var
