"""The rectified-flow sampler: the (shifted) time grid and the Euler, Heun and stochastic loops of the ODE dx/dt = v(x, t)
on ``sde_lib.RectifiedFlow`` (Liu et al., "Flow Straight and Fast", 2022; Lipman et al., "Flow Matching for Generative
Modeling", 2022; the time shift of Esser et al., "Scaling Rectified Flow Transformers", 2024), and an adaptive RK45 run of the
same ODE.

The interpolant x_t = (1 - t) x_0 + t z has the prior N(0, I) at t = 1 and the data at t = 0; the network predicts the
velocity z - x_0.  With the times t_0 = 1 > ... > t_steps = 0 and D_i = t_i - t_{i+1}, one step is

  x' = x - D_i v(x, t_i)                                            order 1, eta = 0: the Euler step
  x  = x - D_i (v(x, t_i) + v(x', t_{i+1})) / 2                      order 2: Heun's correction, unless t_{i+1} = 0
  x' = (1 - eta D_i) x - D_i (1 + eta (1 - t_i)) v + sqrt(2 eta t_i D_i) eps    order 1, eta > 0: the stochastic step

The stochastic step is one Euler-Maruyama step of dx = [-v + (w / 2) score] dtau + sqrt(w) dW in tau = 1 - t, which keeps the
marginals of the interpolant for every w >= 0 (Fokker-Planck), at w = 2 eta t with score = -(x + (1 - t) v) / t, where the
singular 1 / t cancels (include/stk_flow.h).  The last step of every run is the plain Euler step to t = 0, the network's data
prediction x - t v: no noise is left in the sample, and the network is never evaluated at t = 0.

``flow_schedule`` turns a step count into the host coefficients of every launch, in float64 from times rounded to fp32 first
(the network sees exactly the time the coefficients were computed at);  ``flow_sample`` is the loop over any ``v(x, t)``: per
evaluation ONE launch of ``stk_flow_step_f32`` (include/stk_flow.h, csrc/flow.hip), which serves all three forms.  The Heun
correction reads the network's own output of the Euler stage as ``v_prev``, so no slope is ever written; the state and the
Euler point live in two buffers.  ``get_flow_sampler`` binds both to a model the way ``edm.get_edm_sampler`` does;
``order = 'rk45'`` hands dx/dt = v to ``engine.rk45.solve_ivp_rk45`` from t = 1 to ``t_end`` instead and launches no kernel of
the header.

With ``eta = 0`` the only random draw of a whole run is the single ``sde.prior_sampling(shape)``; with ``eta > 0`` one
``torch.randn_like`` per step except the last follows it, in step order: that is part of the interface.  The network
evaluations follow the engine's conventions: ``torch.no_grad``, weights prepared once per run, ``precision`` ('fp16' applies
to the network only: the updates are always fp32).  Everything runs on the device: host tensors raise the package's device
error, there is no CPU path; a library without include/stk_flow.h is refused when the sampler is built.

Out of scope: the likelihood, DPS, PC, ODE, DPM-Solver++, adaptive, parallel and controllable samplers on this family (they
need ``sde()`` at T, singular here, or a data prediction through 1 / alpha), reflow and distillation, minibatch
optimal-transport couplings, loss weights other than 1, Soft Truncation of the time law, a per-sample time in the sampler.
Sample quality (FID) at any step count is unmeasured: no checkpoint trained under this formulation exists.
"""
import math

import numpy as np
import torch

from . import sde_lib
from .engine import lib as stk_lib
from .engine import rk45
from .models import utils as mutils
from .op import _backend

ORDERS = (1, 2, 'rk45')


def _library():
  return mutils.require('has_flow', 'stk_flow.h', 'stk_flow_step_f32', 'the rectified-flow sampler needs')


_fp32, _ptr = mutils.fp32_levels, mutils.optional_ptr


class FlowSchedule:
  """The host record of one run, float64 numpy throughout, every time fp32-representable.  ``times`` [steps + 1] from 1 down
  to 0;  ``delta`` [steps];  ``rows`` [steps, 3], the scalars ``(cx, cv, cn)`` of the step launch of step i (under order 2
  the row of both its stages);  ``nfe``: steps (order 1) or 2 steps - 1 (order 2);  ``launches`` = nfe."""

  def __init__(self, **fields):
    self.__dict__.update(fields)

  def __repr__(self):
    return f'FlowSchedule(steps={self.steps}, order={self.order}, shift={self.shift!r}, eta={self.eta!r}, nfe={self.nfe})'


def _check_order(order):
  if isinstance(order, bool) or not isinstance(order, (int, np.integer, str)) or order not in ORDERS:
    raise ValueError(f'order must be one of {ORDERS}, got {order!r}')
  return order if isinstance(order, str) else int(order)


def flow_schedule(steps, order=1, shift=1.0, eta=0.0):
  """The times and the per-launch coefficients of the rectified-flow sampler (module docstring), as a :class:`FlowSchedule`:
  with u_i = 1 - i / steps, t_i = fp32(shift u_i / (1 + (shift - 1) u_i)), t_0 = 1 and t_steps = 0 exactly;
  D_i = t_i - t_{i+1};  e_i = eta but 0 on the last step;  cx = 1 - e_i D_i, cv = -D_i (1 + e_i (1 - t_i)),
  cn = sqrt(2 e_i t_i D_i).  ValueError naming the option: steps not an integer >= 1, order not 1 or 2 ('rk45' has no
  schedule), shift not positive and finite, eta negative or not finite, eta > 0 with order != 1, two times that coincide in
  fp32, eta max D >= 1 (cx would not be positive)."""
  if isinstance(steps, bool) or not isinstance(steps, (int, np.integer, float)) or not math.isfinite(steps) or \
      int(steps) != steps or steps < 1:
    raise ValueError(f'steps must be an integer >= 1, got {steps!r}')
  steps = int(steps)
  order = _check_order(order)
  try:
    shift, eta = float(shift), float(eta)
  except (TypeError, ValueError):
    raise ValueError(f'shift and eta must be numbers, got {shift!r}, {eta!r}') from None
  if not (shift > 0. and math.isfinite(shift)):
    raise ValueError(f'shift must be positive and finite, got {shift!r}')
  if not (eta >= 0. and math.isfinite(eta)):
    raise ValueError(f'eta must be non-negative and finite, got {eta!r}')
  if eta > 0. and order != 1:
    raise ValueError(f'eta = {eta!r} needs order = 1: the stochastic step is first order, got order = {order!r}')
  if order == 'rk45':
    raise ValueError("order = 'rk45' has no schedule: the solver chooses its own steps (get_flow_sampler)")
  u = 1. - np.arange(steps + 1, dtype=np.float64) / steps
  times = _fp32(shift * u / (1. + (shift - 1.) * u))
  times[0], times[-1] = 1., 0.
  delta = times[:-1] - times[1:]
  if not bool((delta > 0.).all()):
    raise ValueError(f'steps = {steps}, shift = {shift!r}: two times coincide in fp32')
  if eta * float(delta.max()) >= 1.:
    raise ValueError(f'eta = {eta!r} is too large for steps = {steps}: eta max(t_i - t_i+1) must stay below 1')
  e = np.full(steps, eta)
  e[-1] = 0.
  t = times[:-1]
  rows = np.stack([1. - e * delta, -delta * (1. + e * (1. - t)), np.sqrt(2. * e * t * delta)], axis=1)
  nfe = steps if order == 1 else 2 * steps - 1
  return FlowSchedule(steps=steps, order=order, shift=shift, eta=eta, times=times, delta=delta, rows=rows, nfe=nfe, launches=nfe)


def _step(lib, xb, v, v_prev, eps, row, x_out):
  """One launch of stk_flow_step_f32 on contiguous fp32 device tensors.  row: (cx, cv, cn)."""
  cx, cv, cn = (float(c) for c in row)
  with stk_lib.device_guard(xb.device):
    lib.flow_step_f32(xb.data_ptr(), v.data_ptr(), _ptr(v_prev), _ptr(eps), cx, cv, cn, x_out.data_ptr(), xb.numel(),
                      stk_lib.stream_ptr(xb.device))


def flow_sample(velocity_fn, schedule, x, noise_fn=None):
  """The loop: `x` (a contiguous fp32 device tensor drawn from N(0, I), the law at t = 1) is advanced IN PLACE to t = 0 and
  returned.  velocity_fn: any ``v(x, t)`` with t a [B] fp32 tensor (``models.utils.get_flow_model_fn``).  noise_fn(x) -> eps
  of a stochastic step (``torch.randn_like`` where None).  ``schedule.nfe`` evaluations and as many launches."""
  lib = _library()
  mutils.check_inplace_state(x, lib)
  draw = torch.randn_like if noise_fn is None else noise_fn
  steps, B, heun = schedule.steps, x.shape[0], schedule.order == 2
  # the times of all evaluations: t_i, and under order 2 t_{i+1} after it
  levels = np.stack([schedule.times[:-1], schedule.times[1:]], axis=1).reshape(-1)[:schedule.nfe] if heun else schedule.times[:-1]
  cond = mutils.level_conditioning(levels, B, x.device)
  x1 = torch.empty_like(x) if heun and steps > 1 else None
  for i in range(steps):
    row = schedule.rows[i]
    v = mutils.checked_score(velocity_fn, x, cond[2 * i if heun else i], lib)
    if not heun or i == steps - 1:                         # t_{i+1} = 0 under order 2: the Euler point is the result
      eps = None
      if row[2] > 0.:
        eps = draw(x)
        mutils.check_inplace_state(eps, lib, why='the kernel reads it in place')
      _step(lib, x, v, None, eps, row, x)
      continue
    _step(lib, x, v, None, None, row, x1)
    v1 = mutils.checked_score(velocity_fn, x1, cond[2 * i + 1], lib)
    _step(lib, x, v1, v, None, row, x)
  return x


def flow_solve_rk45(velocity_fn, x, t_end=1e-3, rtol=1e-5, atol=1e-5):
  """``(x(t_end), nfev)``: dx/dt = v(x, t) from t = 1 with `engine.rk45.solve_ivp_rk45` -- float64 solver state on the
  device, the network on its float32 cast, as ``sampling.get_ode_sampler`` does."""
  shape = x.shape

  def ode_func(t, y):
    vec_t = torch.full((shape[0],), float(t), dtype=torch.float32, device=x.device)
    return velocity_fn(y.reshape(shape).to(torch.float32), vec_t).reshape(-1).to(torch.float64)

  y, nfev = rk45.solve_ivp_rk45(ode_func, (1., float(t_end)), x.reshape(-1).to(torch.float64), rtol=rtol, atol=atol)
  return y.reshape(shape).to(torch.float32), nfev


def get_flow_sampler(config, sde, shape, inverse_scaler, steps=50, order=1, shift=1.0, eta=0.0, t_end=1e-3, rtol=1e-5,
                     atol=1e-5, device='cuda', precision='fp32'):
  """``flow_sampler(model) -> (samples, nfe)``: the rectified-flow sampler over `steps` steps from t = 1 to 0 with
  ``nfe = steps`` (order 1) or ``2 steps - 1`` (order 2, Heun), or, under ``order = 'rk45'``, the adaptive solve from 1 to
  `t_end` at `rtol`, `atol` with the solver's ``nfev`` (`steps`, `shift`, `eta` do not apply).  precision='fp16': every network
  evaluation runs in the engine's fp16 mode (models.utils.precision); not under 'rk45'.  ValueError for an `sde` other than
  sde_lib.RectifiedFlow, for a config the family refuses (models.utils.check_flow_config) and for invalid options;
  NotImplementedError for a library without include/stk_flow.h -- all when the sampler is built."""
  lib = _library()
  if not isinstance(sde, sde_lib.RectifiedFlow):
    raise ValueError(f'the rectified-flow sampler needs sde_lib.RectifiedFlow (config.training.sde = \'rectified_flow\'), got '
                     f'{type(sde).__name__}')
  mutils.check_flow_config(config)
  mutils.check_precision(precision)
  order = _check_order(order)
  adaptive = order == 'rk45'
  if adaptive:
    if precision != 'fp32':
      raise ValueError(f"precision={precision!r} is not supported under order = 'rk45': RK45 at rtol = atol = 1e-5 sits below "
                       f"the fp16-level noise of the velocity, and its step controller's behaviour there is unmeasured; use "
                       f"precision='fp32' or order = 1 or 2")
    t_end, rtol, atol = float(t_end), float(rtol), float(atol)
    if not 0. <= t_end < 1.:
      raise ValueError(f't_end must lie in [0, 1), got {t_end!r}')
    if not (rtol > 0. and atol > 0.):
      raise ValueError(f'rtol and atol must be positive, got {rtol!r}, {atol!r}')
    schedule = None
  else:
    schedule = flow_schedule(steps, order=order, shift=shift, eta=eta)

  def flow_sampler(model):
    with mutils.sampling_run(model, precision):
      velocity_fn = mutils.get_flow_model_fn(config, model, train=False)
      x = sde.prior_sampling(shape).to(device).contiguous()
      _backend.check(x, lib)
      if adaptive:
        x, nfe = flow_solve_rk45(velocity_fn, x, t_end, rtol, atol)
        return inverse_scaler(x), nfe
      x = flow_sample(velocity_fn, schedule, x)
      return inverse_scaler(x), schedule.nfe

  return flow_sampler


def sampling_options(config):
  """(steps, order, shift, eta, t_end, rtol, atol) of ``config.sampling.flow_steps / flow_order / flow_shift / flow_eta /
  flow_t_end / flow_rtol / flow_atol``: 50, 1, 1, 0, 1e-3, 1e-5 and 1e-5 where a key is absent."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  return (read('flow_steps', 50), read('flow_order', 1), read('flow_shift', 1.0), read('flow_eta', 0.0), read('flow_t_end', 1e-3),
          read('flow_rtol', 1e-5), read('flow_atol', 1e-5))
